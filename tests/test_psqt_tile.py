"""The bucket-major PSQT tile of ft_slices on the host (DESIGN.md §4.2 "PSQT tile").

The index map (fishnet_amd/csrc/psqt_tile.h): tests/psqt_tile_host.cpp is built
with the host compiler and replays the fill for the chess / atomic (704 rows)
and crazyhouse (864 rows) geometries; see its header for what it checks.

The bank model (tools/lds_bank_sim.py): on seeded lists with one bucket per
pass the four gathers of a wave-pass cost fewer modelled LDS cycles
bucket-major than row-major.  Only the ordering is asserted; the values are
printed (pytest -s)."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_index_map(tmp_path):
    exe = tmp_path / "psqt_tile_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests/psqt_tile_host.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "704", "864"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert not [ln for ln in out if ln.startswith("error")], out[:10]
    geoms = [[int(v) for v in ln.split()[1::2][:4]] + [[int(v) for v in ln.split()[9:]]] for ln in out
             if ln.startswith("geom")]
    banks = [4 * b for b in range(8)]  # bucket b's rows start on bank 4 b: one bucket's rows cover all 32
    assert geoms == [[704, 708, 8 * 708, 2 * 708, banks], [864, 868, 8 * 868, 2 * 868, banks]]
    # two 16-byte chunks per thread of the 1024: the fill needs no third load
    assert all(g[3] <= 2048 for g in geoms)


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("lds_bank_sim", os.path.join(ROOT, "tools/lds_bank_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rows", [11, 21, 29])
@pytest.mark.parametrize("geom", [704, 864])
def test_bank_model_orders_the_layouts(sim, rows, geom):
    rng = np.random.default_rng(1000 * geom + rows)
    stride = sim.psqt_stride(geom)
    assert stride == {704: 708, 864: 868}[geom]
    tot = {k: 0 for k in sim.PSQT_LAYOUTS}
    passes = 400
    for _ in range(passes):
        lists = np.full((8, 32), geom, np.int64)  # padding names the zero row
        for j in range(8):
            lists[j, :rows] = rng.choice(geom, rows, replace=False)
        bk = np.full(8, int(rng.integers(0, 8)))  # one bucket per pass
        for k in sim.PSQT_LAYOUTS:
            c = sim.psqt_pass_cycles(lists, bk, k, stride)
            assert c >= 8
            tot[k] += c
    print(f"rows {rows} geometry {geom}: LDS cycles per wave-pass row-major {tot['row-major'] / passes:.1f}, "
          f"bucket-major {tot['bucket-major'] / passes:.1f} (8 = conflict-free)")
    assert tot["bucket-major"] < tot["row-major"]


def test_bank_model_on_known_passes(sim):
    """Hand-checked prices: one row everywhere broadcasts (8 cycles either way); rows 0, 4, 8, ... in
    one bucket share a bank row-major (8 (row mod 4) + bucket) and spread bucket-major."""
    same = np.full((8, 32), 704, np.int64)
    bk = np.zeros(8, np.int64)
    assert sim.psqt_pass_cycles(same, bk, "row-major") == 8 == sim.psqt_pass_cycles(same, bk, "bucket-major")
    i, t, j = np.arange(8)[:, None, None], np.arange(8)[None, :, None], np.arange(4)[None, None, :]
    lists = (4 * (8 * (i % 4) + t) + 128 * j).reshape(8, 32)  # entry 4 t + j of item i
    row = sim.psqt_pass_cycles(lists, bk, "row-major")
    buc = sim.psqt_pass_cycles(lists, bk, "bucket-major")
    # a half's gather j reads 32 distinct multiples of 4: one bank row-major (32 cycles), 8 banks bucket-major (4)
    assert row == 4 * 2 * 32 and buc == 4 * 2 * 4

"""CPU tests of bench.py's algorithmic-byte accounting."""
import json
import os

import numpy as np
import pytest

import bench
import fishnet_amd as F


def test_rows_scratch_counts_both_perspectives():
    pos = np.stack([F.pos_from_fen("4k3/8/8/8/8/8/8/4K3 w - - 0 1"),
                    F.pos_from_fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1")])
    assert bench.rows_scratch(bench.boards_of(pos)).tolist() == [4, 64]


def test_rows_incremental_quiet_capture_king_move():
    fen = "4k3/8/8/3p4/4P3/8/8/4K3 w - - 0 1"
    pos = F.game_positions(fen, "e4d5 e8d7 e1e2")
    b = bench.boards_of(pos)
    has = np.array([False, True, True, True])
    rows = bench.rows_incremental(b, b[[0, 0, 1, 2]], has)
    # root: refresh 4 pieces x 2; capture: -P(e4) +P(d5) -p(d5) = 3 per perspective;
    # black king move: black refreshes (3 pieces), white -k +k = 2; white king move: 3 + 2
    assert rows.tolist() == [8, 6, 5, 5]


def test_default_arguments_match_the_driver_contract(monkeypatch):
    """No flags: one GPU, a run of minutes at most; the untimed settle phase
    runs before the W warm-up steps and is reported, not counted."""
    monkeypatch.setattr("sys.argv", ["bench.py"])
    a = bench.parse_args()
    assert (a.gpus, a.workload, a.positions, a.hd) == (1, "positions", 1_000_000, 1024)
    assert a.steps >= 1 and a.warmup >= 1 and 0 < a.settle_s <= 1.0
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--settle-s", "0"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.settle_s) == (20, 5, 0.0)
    # a plain run is the headline alone: everything beside it waits for --full
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float64_within_the_budget(tmp_path, monkeypatch):
    """Small outputs are written whole (int32 exactly, as float64); past the
    budget every array is cut to the same seeded sample from run to run."""
    ps = np.arange(-500, 500, dtype=np.int32) * 2_000_003
    po = np.arange(1000, dtype=np.int32)
    w = bench.dump_outputs(str(tmp_path / "a"), {"psqt": ps, "positional": po})
    assert w == {"psqt": {"elements": 1000, "of": 1000}, "positional": {"elements": 1000, "of": 1000}}
    got = np.load(tmp_path / "a" / "psqt.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.int64), ps.astype(np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "positional.npy"), po)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096 + 2 * 1024)
    for d in ("b", "c"):
        w = bench.dump_outputs(str(tmp_path / d), {"psqt": ps, "positional": po})
    assert w["psqt"] == {"elements": 256, "of": 1000}
    b, c = np.load(tmp_path / "b" / "psqt.npy"), np.load(tmp_path / "c" / "psqt.npy")
    assert np.array_equal(b, c) and len(b) == 256 and np.isin(b, ps).all()
    size = sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c"))
    assert size <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_their_outputs(tmp_path, monkeypatch, capsys, oracle_big):
    """A plain run: --steps timed steps, the result line with ms_per_step,
    nothing beside the headline; the dumped arrays are the evaluation of the
    seeded inputs (the oracle's, bit for bit)."""
    from fishnet_amd import dist as D
    n = 3000  # more than one block of the FT kernel, no multiple of its tile
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-s", "0",
                                     "--positions", str(n), "--dump-outputs", str(tmp_path / "out")])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["steps"], line["warmup"], line["n_gpus"], line["full"]) == (3, 1, 1, False)
    assert line["unit"] == "positions/s" and line["higher_is_better"] is True and line["dtype"] == "int16"
    assert line["ms_per_step"] > 0 and abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["roofline"]["kernel_avg_ms"] > 0
    assert all(line[k] is None for k in ("cpu_baseline", "parity_spot_check", "host_api", "gathered"))
    assert "extra" not in line
    assert sorted(os.listdir(tmp_path / "out")) == ["positional.npy", "psqt.npy"]
    ps, po, rc = oracle_big.eval_packed(F.random_playouts(D.shard_seed(1, 0), n, 0, 160))
    assert rc == 0
    got_ps, got_po = np.load(tmp_path / "out" / "psqt.npy"), np.load(tmp_path / "out" / "positional.npy")
    assert got_ps.dtype == got_po.dtype == np.float64
    assert np.array_equal(got_ps, ps) and np.array_equal(got_po, po)


def test_resource_fractions_use_the_spec_peaks():
    """VALU issue, LDS-busy and bytes past L2 ((2 FETCH_SIZE + WRITE_SIZE) KiB,
    the gfx950 correction) of one launch over its time, against the 2.4 GHz
    spec peaks; the roofline's frac is the largest."""
    t = 1e-3
    c = {"SQ_INSTS_VALU": 0.5 * bench.VALU_PEAK * t, "SQ_LDS_IDX_ACTIVE": 0.25 * bench.LDS_PEAK * t,
         "FETCH_SIZE": 1e5, "WRITE_SIZE": 2e5}
    fr = bench.resource_fractions(c, t)
    assert fr["valu"]["frac"] == 0.5 and fr["lds"]["frac"] == 0.25
    assert fr["hbm"]["bytes"] == (2 * 1e5 + 2e5) * 1024
    assert abs(fr["hbm"]["frac"] - fr["hbm"]["bytes"] / t / 1e9 / bench.HBM_PEAK_GBS) < 1e-4
    assert max(fr, key=lambda k: fr[k]["frac"]) == "valu"

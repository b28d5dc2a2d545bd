"""SWAR row sums decided per 64-column slice on the GPU: forced
slice masks on ordinary nets and the heavy-tailed synthetic nets, whose heavy
slices run packed int16 rows beside SWAR slices in one launch.  Every result
is compared with the CPU oracle on the same bytes (bit-exact) and with the
library's own full-mask / all-packed run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet, VariantOracleNet
from tests import refpy
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CZH, ATOMIC = F.VARIANT_CRAZYHOUSE, F.VARIANT_ATOMIC
SMALL = (1001, 128, 0)  # the small net of the dual calls, its own mask 0b10


def star_groups(seed: int, cap: int = 20000):
    """Positions with their children (STAR groups), whole groups up to `cap` positions."""
    pos, off = F.random_playouts(seed, 20, 0, 40, mode=N.PLAYOUT_CHILDREN, threads=8)
    g = int(np.searchsorted(off, cap, side="right")) - 1
    return pos[: off[g]], off[: g + 1]


class World:
    """Evaluators, oracles, inputs and the oracle's answers, made once."""

    def __init__(self):
        self.nets, self.inputs, self.answers = {}, {}, {}

    def net(self, seed, hd, flags):
        key = (seed, hd, flags)
        if key not in self.nets:
            data = F.synthesize_net(seed, hd, flags)
            ev = F.Evaluator(F.Net.from_bytes(data), 0)
            ev.set_ft_impl(N.FT_SLICED)  # positions calls through ft_slices at any size
            self.nets[key] = (ev, OracleNet(data), data)
        return self.nets[key]

    def input(self, name):
        if name not in self.inputs:
            self.inputs[name] = {
                "pos": lambda: (F.random_playouts(71, 20000, threads=8), None),
                "chain": lambda: F.random_playouts(72, 200, 0, 60, mode=N.PLAYOUT_PLIES, threads=8),
                "star": lambda: star_groups(73),
                # early plies: 28-32 pieces, the sums of the heavy columns reach their limits
                "early_pos": lambda: (F.random_playouts(74, 20000, 0, 40, threads=8), None),
                "early_chain": lambda: F.random_playouts(75, 200, 0, 40, mode=N.PLAYOUT_PLIES, threads=8),
                "early_star": lambda: star_groups(76),
            }[name]()
        return self.inputs[name]

    def oracle(self, key, name):
        if (key, name) not in self.answers:
            ps, po, rc = self.net(*key)[1].eval_packed(self.input(name)[0], threads=8)
            assert rc == 0
            self.answers[(key, name)] = (ps, po)
        return self.answers[(key, name)]

    def close(self):
        for ev, _, _ in self.nets.values():
            ev.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def run(ev, w, name):
    pos, off = w.input(name)
    if off is None:
        return ev.eval_positions(pos)
    return ev.eval_groups(pos, off, N.GROUP_STAR if name.endswith("star") else N.GROUP_CHAIN)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


FORCED = [(7, 128, 0b01), (7, 128, 0b10),
          (1, 1024, 0x5555), (1, 1024, 0x0001), (1, 1024, 0xFFFE), (1, 1024, 0x8001),
          (10, 3072, 0x84210F0F5A5A)]


@pytest.mark.parametrize("seed,hd,mask", FORCED, ids=[f"{hd}-{mask:#x}" for _, hd, mask in FORCED])
def test_forced_masks_on_ordinary_nets(world, seed, hd, mask):
    """Every slice of an ordinary net is eligible; any mask gives the oracle's
    and the full mask's results on ft_slices, ft_segments CHAIN / STAR and the
    dual call, and is reported back."""
    key = (seed, hd, 0)
    ev, _, _ = world.net(*key)
    ns = hd // 64
    full = (1 << ns) - 1
    assert ev.swar_slices() == (full, full, ns)
    assert 0 < mask < full and (hd != 3072 or (mask >> 32 and mask & 0xFFFFFFFF))
    names = ("pos", "chain", "star")
    ref = {n: run(ev, world, n) for n in names}  # the full mask
    small = world.net(*SMALL)[0] if hd == 1024 else None
    gpos, goff = world.input("chain")
    try:
        if small:
            small.set_swar_slices(0b10)
            assert small.swar_slices()[1] == 0b10
            dual_ref = ev.eval_groups_dual(small, gpos, goff, N.GROUP_CHAIN)
        ev.set_swar_slices(mask)
        assert ev.swar_slices() == (full, mask, ns) and ev.swar()[0] is True
        for n in names:
            got = run(ev, world, n)
            assert same(got, world.oracle(key, n)), f"{n}: mask {mask:#x} differs from the oracle"
            assert same(got, ref[n]), f"{n}: mask {mask:#x} differs from the full mask"
        if small:
            d = ev.eval_groups_dual(small, gpos, goff, N.GROUP_CHAIN)
            assert same(d[:2], world.oracle(key, "chain")) and same(d[2:], world.oracle(SMALL, "chain"))
            assert all(np.array_equal(a, b) for a, b in zip(d, dual_ref))
        with pytest.raises(F.FnnueError) as e:
            ev.set_swar_slices(1 << ns)
        assert e.value.name == "FNNUE_E_ARG"
        assert ev.swar_slices()[1] == mask
    finally:
        ev.set_swar(True)
        if small:
            small.set_swar(True)
    assert ev.swar_slices()[1] == full


def heavy_sums(data: bytes, pos: np.ndarray):
    """True (unwrapped) accumulator sums of the heavy columns over both
    perspectives of `pos`: (second-half columns' sums, first-half columns' sums)."""
    net = refpy.RefNet(data)
    half = net.hd // 2
    cols = np.nonzero(np.abs(net.w).min(axis=0) >= 500)[0]
    assert len(cols) == len(range(1, net.hd // 64, 3))
    sums = []
    for p in pos:
        board = np.zeros(64, np.uint8)
        board[0::2], board[1::2] = p[:32] & 15, p[:32] >> 4
        board = [int(x) for x in board]
        pieces = [(s, pc) for s, pc in enumerate(board) if pc]
        for persp, ksq in ((0, board.index(6)), (1, board.index(14))):
            idx = [refpy.feature(persp, s, pc, ksq) for s, pc in pieces]
            sums.append(net.bias[cols] + net.w[np.ix_(idx, cols)].sum(axis=0))
    sums = np.array(sums)
    return sums[:, cols >= half], sums[:, cols < half]


@pytest.mark.parametrize("hd", [512, 1024])
def test_heavy_net_runs_mixed_slices(world, hd):
    """FNNUE_SYNTH_HEAVY: the slices with s % 3 == 1 fail the bound and run
    packed rows, the others SWAR rows, in one launch; results equal the oracle
    and the all-packed run on inputs that reach the limits."""
    key = (5, hd, N.SYNTH_HEAVY)
    ev, _, data = world.net(*key)
    ns = hd // 64
    light = sum(1 << s for s in range(ns) if s % 3 != 1)
    assert ev.swar_slices() == (light, light, ns)
    assert ev.swar() == (True, int(F.Net.from_bytes(data).slice_bounds().max()))
    with pytest.raises(F.FnnueError) as e:
        ev.set_swar_slices(light | 0b10)
    assert e.value.name == "FNNUE_E_ARCH"
    assert ev.swar_slices()[1] == light
    # the inputs reach the limits: a doubled second-half sum past 2^15, a first-half sum past 2^15
    second, first = heavy_sums(data, world.input("early_pos")[0][:3000])
    assert np.abs(second).max() > 1 << 14
    assert np.abs(first).max() > 1 << 15
    names = ("early_pos", "early_chain", "early_star")
    mixed = {n: run(ev, world, n) for n in names}
    ev.set_swar(False)
    try:
        assert ev.swar_slices()[1] == 0 and ev.swar()[0] is False
        packed = {n: run(ev, world, n) for n in names}
    finally:
        ev.set_swar(True)
    assert ev.swar_slices()[1] == light
    for n in names:
        assert same(mixed[n], world.oracle(key, n)), f"{n}: mixed slices differ from the oracle"
        assert same(mixed[n], packed[n]), f"{n}: mixed slices differ from packed rows"


@pytest.mark.parametrize("variant", [CZH, ATOMIC])
def test_heavy_variant_nets(variant):
    data = F.synthesize_variant_net(5, 256, variant, N.SYNTH_HEAVY)
    ev, on = F.Evaluator(F.Net.from_bytes_variant(data, variant), 0), VariantOracleNet(data, variant)
    try:
        assert ev.swar_slices() == (0b1101, 0b1101, 4)
        pos = F.random_vpositions(77, variant, 20000, 40)
        ops, opo, rc = on.eval_packed(pos, threads=8)
        assert rc == 0 and same(ev.eval_vpositions(pos), (ops, opo))
        gpos, off = F.random_vpositions(78, variant, 200, 40, mode=N.PLAYOUT_PLIES)
        ops, opo, rc = on.eval_packed(gpos, threads=8)
        mixed = ev.eval_vgroups(gpos, off, N.GROUP_CHAIN)
        assert rc == 0 and same(mixed, (ops, opo))
        ev.set_swar(False)
        assert same(ev.eval_vpositions(pos), on.eval_packed(pos, threads=8)[:2]) and same(
            ev.eval_vgroups(gpos, off, N.GROUP_CHAIN), mixed)
    finally:
        ev.close()


CHILD = """
import fishnet_amd as F
from fishnet_amd import _native as N
ev = F.Evaluator(F.Net.from_bytes(F.synthesize_net(5, 512, N.SYNTH_HEAVY)), 0)
print("slices", *ev.swar_slices(), int(ev.swar()[0]))
ev.close()
"""


def test_environment_keeps_swar_off_in_a_child_process():
    env = dict(os.environ, FNNUE_SWAR="0")
    out = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, check=True, capture_output=True,
                         text=True, timeout=120).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("slices ")][-1].split()
    light = sum(1 << s for s in range(8) if s % 3 != 1)
    assert [int(v) for v in line[1:]] == [light, 0, 8, 0]  # eligible unchanged, nothing enabled

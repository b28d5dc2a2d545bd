"""GPU parity of ft_slices at the edges of its pass claiming (DESIGN.md §4.2 "Claimed passes"):
the first two passes of a wave are its own, every later pass of the unit is claimed from an LDS
counter.  Copies of one position give one king block per perspective with lists of equal length,
so the unit's length in passes is exact: one pass (fifteen idle waves), a one-item partial pass,
sixteen passes, the 32-pass boundary where the counter takes over, and several counter rounds
with a partial last pass.  Mixed lengths make the faster waves claim more; a cut block starts
several counters.  Every result (psqt: slice 0's copy of the loop; positional: all slices) is
compared bit-exactly with the CPU oracle."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet, VariantOracleNet
from tests.conftest import net_bytes

pytestmark = pytest.mark.gpu

CZH, ATOMIC = F.VARIANT_CRAZYHOUSE, F.VARIANT_ATOMIC
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
FENS = {"32-piece": START, "3-piece": "8/8/4k3/8/8/3K4/4P3/8 w - - 0 1"}  # 3 pieces: one row per item
COPIES = [1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 264, 1000, 2055]
VFENS = {CZH: "r1bqk2r/ppp2ppp/2n5/4p3/4P3/5N2/PPP2PPP/R1BQK2R[NBPnbp] w KQkq - 0 1",  # six in the pockets
         ATOMIC: "r1bqkb1r/ppp2ppp/2n2n2/4p3/4P3/5N2/PPP2PPP/RNBQKB1R w KQkq - 0 1"}


@pytest.fixture(scope="module")
def net():
    data = net_bytes(1, 1024, 0)
    ev = F.Evaluator(F.Net.from_bytes(data), 0)
    ev.set_ft_impl(N.FT_SLICED)  # small calls would otherwise take the gather kernel
    yield ev, OracleNet(data)
    ev.close()


@pytest.fixture(scope="module")
def one(net):
    """The oracle's answer for one copy of each position."""
    out = {}
    for name, fen in FENS.items():
        p = F.pos_from_fen(fen)
        ps, po, rc = net[1].eval_packed(p[None, :])
        assert rc == 0
        out[name] = (p, int(ps[0]), int(po[0]))
    return out


@pytest.fixture(scope="module")
def playouts(net):
    pos = F.random_playouts(91, 5000, threads=8)
    ps, po, rc = net[1].eval_packed(pos, threads=8)
    assert rc == 0
    return pos, ps, po


def assert_copies(ev, one, name, copies):
    p, ops, opo = one[name]
    ps, po = ev.eval_positions(np.repeat(p[None, :], copies, axis=0))
    assert ps.shape == (copies,) and po.shape == (copies,)
    bad = np.nonzero((ps != ops) | (po != opo))[0]
    assert len(bad) == 0, f"{name} x {copies}: {len(bad)} mismatches, first {bad[:5]}"


@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", list(FENS))
def test_unit_length_edges(net, one, name, copies):
    assert_copies(net[0], one, name, copies)


def test_passes_of_uneven_cost(net, playouts):
    """Mixed list lengths within every unit, and the same batch reversed: another plan, the same
    results position by position."""
    pos, ops, opo = playouts
    ps, po = net[0].eval_positions(pos)
    assert np.array_equal(ps, ops) and np.array_equal(po, opo)
    ps, po = net[0].eval_positions(np.ascontiguousarray(pos[::-1]))
    assert np.array_equal(ps[::-1], ops) and np.array_equal(po[::-1], opo)


def test_cut_block(net, one):
    """10,000 copies of the start position: three units of one block, each with its own counter."""
    assert_copies(net[0], one, "32-piece", 10000)


@pytest.mark.parametrize("copies", [9, 257, 2055])
@pytest.mark.parametrize("name", list(FENS))
@pytest.mark.parametrize("body", ["packed", "mixed"])
def test_packed_and_mixed_bodies(net, one, body, name, copies):
    ev = net[0]
    full = (1 << 16) - 1
    try:
        if body == "packed":
            ev.set_swar(False)
            assert ev.swar_slices()[1] == 0
        else:
            ev.set_swar_slices(0x5555)  # alternating: SWAR and packed slices in one launch
            assert ev.swar_slices()[1] == 0x5555
        assert_copies(ev, one, name, copies)
    finally:
        ev.set_swar(True)
    assert ev.swar_slices()[1] == full


@pytest.mark.parametrize("variant", [CZH, ATOMIC], ids=["crazyhouse", "atomic"])
def test_variant_geometries(variant):
    data = F.synthesize_variant_net(3, 1024, variant, 0)
    ev, on = F.Evaluator(F.Net.from_bytes_variant(data, variant), 0), VariantOracleNet(data, variant)
    try:
        p = F.vpos_from_fen(variant, VFENS[variant])
        ops, opo, rc = on.eval_packed(p[None, :])
        assert rc == 0
        for copies in (257, 2055):
            ps, po = ev.eval_vpositions(np.repeat(p[None, :], copies, axis=0))
            bad = np.nonzero((ps != ops[0]) | (po != opo[0]))[0]
            assert ps.shape == (copies,) and len(bad) == 0, f"x {copies}: {len(bad)} mismatches, first {bad[:5]}"
        pos = F.random_vpositions(92, variant, 3000, 160)
        ops, opo, rc = on.eval_packed(pos, threads=8)
        ps, po = ev.eval_vpositions(pos)
        assert rc == 0 and np.array_equal(ps, ops) and np.array_equal(po, opo)
    finally:
        ev.close()

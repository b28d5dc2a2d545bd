"""GPU parity of ft_slices over the work-budget unit table (slice_units.h), bit-exact against the
oracle, on batches that reach the table's edges: one king block cut into several units, batches
whose king blocks all hold a handful of items, a mixed batch whose largest block is cut and the
others are not, and the dual call (the second unit table of the segment plan shares the scan)."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet
from tests.conftest import net_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets():
    big, small = net_bytes(1, 1024, 0), net_bytes(7, 128, 0)
    evs = (F.Evaluator(F.Net.from_bytes(big), 0), F.Evaluator(F.Net.from_bytes(small), 0))
    yield evs[0], OracleNet(big), evs[1], OracleNet(small)
    for ev in evs:
        ev.close()


@pytest.fixture(scope="module")
def playouts(nets):
    pos = F.random_playouts(1, 20000, threads=8)
    ops, opo, rc = nets[1].eval_packed(pos, threads=8)
    assert rc == 0
    return pos, ops, opo


def sliced(ev, pos):
    ev.set_ft_impl(N.FT_SLICED)
    try:
        return ev.eval_positions(pos)
    finally:
        ev.set_ft_impl(N.FT_AUTO)


def assert_same(ev, on, pos):
    ps, po = sliced(ev, pos)
    ops, opo, rc = on.eval_packed(pos, threads=8)
    assert rc == 0
    bad = np.nonzero((ps != ops) | (po != opo))[0]
    assert len(bad) == 0, f"{len(bad)} mismatches, first {bad[:5]}"


@pytest.mark.parametrize("fen,copies", [
    ("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", 10000),   # 32 pieces: 3 units of one block
    ("r4rk1/1pp1qppp/p1np1n2/2b1p1B1/2B1P1b1/P1NP1N2/1PP1QPPP/R4RK1 w - - 0 10", 10007),
    ("8/8/4k3/8/8/3K4/4P3/8 w - - 0 1", 9999),                             # 3 pieces: one unit per block
])
def test_copies_of_one_position(nets, fen, copies):
    ev, on = nets[0], nets[1]
    pos = np.repeat(F.pos_from_fen(fen)[None, :], copies, axis=0)
    assert_same(ev, on, pos)


def test_every_king_block_tiny(nets):
    """Kings on every square pair of a coarse grid: all 32 blocks hold a few items, one unit each,
    and the table's last row is partial."""
    ev, on = nets[0], nets[1]
    fens = []
    for wk in range(64):
        for bk in range(0, 64, 5):
            if max(abs(wk // 8 - bk // 8), abs(wk % 8 - bk % 8)) < 2:
                continue
            board = [["1"] * 8 for _ in range(8)]
            board[7 - wk // 8][wk % 8] = "K"
            board[7 - bk // 8][bk % 8] = "k"
            ranks = ["".join(r) for r in board]
            for k in range(8, 0, -1):  # "1" * k -> "k"
                ranks = [r.replace("1" * k, str(k)) for r in ranks]
            fens.append("/".join(ranks) + " w - - 0 1")
    pos = np.stack([F.pos_from_fen(f) for f in fens])
    assert 500 < len(pos) < 1000
    assert_same(ev, on, pos)
    assert_same(ev, on, pos[:37])


def test_random_playouts_sliced(nets, playouts):
    pos, ops, opo = playouts
    ps, po = sliced(nets[0], pos)
    assert np.array_equal(ps, ops) and np.array_equal(po, opo)


def test_random_playouts_several_table_rows(nets):
    """120,000 positions: about 25 units, the largest block cut in ten, three snake rows."""
    assert_same(nets[0], nets[1], F.random_playouts(3, 120_000, threads=8))


def test_random_playouts_gather_agrees(nets, playouts):
    pos, ops, opo = playouts
    ev = nets[0]
    ev.set_ft_impl(N.FT_GATHER)
    try:
        ps, po = ev.eval_positions(pos)
    finally:
        ev.set_ft_impl(N.FT_AUTO)
    a, b = sliced(ev, pos)
    assert np.array_equal(ps, a) and np.array_equal(po, b)
    assert np.array_equal(ps, ops) and np.array_equal(po, opo)


def test_dual_call_on_games(nets):
    eb, ob, es, os_ = nets
    pos, off = F.random_playouts(2, 300, mode=N.PLAYOUT_PLIES, threads=8)
    ps, po, ps2, po2 = eb.eval_groups_dual(es, pos, off, N.GROUP_CHAIN)
    for on, x, y in ((ob, ps, po), (os_, ps2, po2)):
        ops, opo, rc = on.eval_packed(pos, threads=8)
        assert rc == 0 and np.array_equal(x, ops) and np.array_equal(y, opo)

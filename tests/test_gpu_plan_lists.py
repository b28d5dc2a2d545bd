"""plan_scatter builds both feature lists of a position from one board walk (plan_lists.h): the
sliced pipeline at HD 1024 against the oracle, bit-exact in psqt and positional, on the boards that
reach the builder's edges (tests/test_plan_lists.py has the same boards on the host) and on batch
sizes around the workgroup of 1024 positions.

Boards: two bare kings with each king on files a-d / e-h and the kings in the same / in different
half boards; 32 pieces; all other pieces on even files only and on odd files only (one parity run
holds the other king alone or nothing); all pieces in one half board.  Each with either side to
move, at 1, 2, 3, 9 and 257 copies: an item's parity within its king block decides which run comes
first, and 257 copies leave partial passes of 8 items."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N

pytestmark = pytest.mark.gpu


def fen_of(pieces, stm):
    """pieces: {square 0..63 (a1 = 0): letter}."""
    ranks = []
    for r in range(7, -1, -1):
        row, gap = "", 0
        for f in range(8):
            c = pieces.get(8 * r + f)
            if c is None:
                gap += 1
            else:
                row += (str(gap) if gap else "") + c
                gap = 0
        ranks.append(row + (str(gap) if gap else ""))
    return "/".join(ranks) + f" {stm} - - 0 1"


def filled(rng, wk, bk, count, squares):
    """Kings on wk / bk and `count` other pieces on squares drawn from `squares` (pawns on ranks 2-7)."""
    pieces = {wk: "K", bk: "k"}
    free = [s for s in squares if s not in pieces]
    for s in rng.permutation(free)[:count]:
        s = int(s)
        pieces[s] = str(rng.choice(list("NBRQnbrq" + ("Pp" if 8 <= s < 56 else ""))))
    return pieces


def edge_boards():
    rng = np.random.default_rng(11)
    every = range(64)
    boards = []
    # bare kings: files a-d / e-h in all four combinations, same and different half boards
    for wk, bk in ((1, 26), (1, 30), (6, 26), (6, 30), (1, 58), (1, 62), (6, 58), (6, 62), (36, 59), (35, 60)):
        boards.append({wk: "K", bk: "k"})
    boards.append(filled(rng, 4, 60, 30, every))                                    # 32 pieces
    boards.append(filled(rng, 27, 36, 30, every))
    boards.append(filled(rng, 2, 61, 30, every))
    for wk, bk in ((4, 60), (3, 59), (4, 59), (3, 60)):
        boards.append(filled(rng, wk, bk, 14, [s for s in every if s % 2 == 0]))    # even files only
        boards.append(filled(rng, wk, bk, 14, [s for s in every if s % 2 == 1]))    # odd files only
    boards.append(filled(rng, 4, 25, 12, range(32)))                                # lower half board only
    boards.append(filled(rng, 2, 13, 30, range(32)))
    boards.append(filled(rng, 60, 34, 12, range(32, 64)))                           # upper half board only
    boards.append(filled(rng, 37, 58, 30, range(32, 64)))
    boards.append(filled(rng, 4, 60, 13, range(32)))                                # kings apart, pieces below
    return [fen_of(b, stm) for b in boards for stm in "wb"]


@pytest.fixture(scope="module")
def ev(gpu_eval):
    gpu_eval.set_ft_impl(N.FT_SLICED)
    yield gpu_eval
    gpu_eval.set_ft_impl(N.FT_AUTO)


@pytest.fixture(scope="module")
def edges(oracle_big):
    pos = np.stack([F.pos_from_fen(f) for f in edge_boards()])
    ops, opo, rc = oracle_big.eval_packed(pos, threads=8)
    assert rc == 0
    return pos, ops, opo


@pytest.fixture(scope="module")
def playouts(oracle_big):
    pos = F.random_playouts(23, 5000, threads=8)
    ops, opo, rc = oracle_big.eval_packed(pos, threads=8)
    assert rc == 0
    return pos, ops, opo


def assert_exact(ev, pos, ops, opo):
    ps, po = ev.eval_positions(pos)
    bad = np.nonzero((ps != ops) | (po != opo))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(pos)} differ, first {bad[:5]}"


@pytest.mark.parametrize("copies", [1, 2, 3, 9, 257])
def test_edge_boards_in_copies(ev, edges, copies):
    pos, ops, opo = edges
    assert len(pos) == 52
    assert_exact(ev, np.repeat(pos, copies, axis=0), np.repeat(ops, copies), np.repeat(opo, copies))


@pytest.mark.parametrize("copies", [1, 2, 3, 9, 257])
def test_each_edge_board_alone(ev, edges, copies):
    """One board per call: every item of the batch is in the same two king blocks, so consecutive
    items alternate in parity."""
    pos, ops, opo = edges
    for i in range(0, len(pos), 1 if copies < 9 else 7):
        assert_exact(ev, np.repeat(pos[i:i + 1], copies, axis=0), np.repeat(ops[i], copies), np.repeat(opo[i], copies))


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_batches_at_workgroup_edges(ev, playouts, n):
    pos, ops, opo = playouts
    assert_exact(ev, pos[:n], ops[:n], opo[:n])


def test_playouts_forward_and_reversed(ev, playouts):
    pos, ops, opo = playouts
    assert_exact(ev, pos, ops, opo)
    assert_exact(ev, pos[::-1], ops[::-1], opo[::-1])


def test_invalid_position_in_the_middle(ev, playouts):
    """The host call fails with FNNUE_E_POSITION and names the position; on the device entry point
    the error is latched, the invalid position gives 0 / 0 and every other row its exact result."""
    import torch
    pos, ops, opo = playouts
    n, hole = 2049, 1030
    bad = pos[:n].copy()
    bad[hole, :32] = 0  # no kings
    with pytest.raises(F.FnnueError) as e:
        ev.eval_positions(bad)
    assert e.value.name == "FNNUE_E_POSITION" and f"index {hole}" in str(e.value)
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(bad).to(dev)
    d_ps = torch.full((n,), 77, dtype=torch.int32, device=dev)
    d_po = torch.full((n,), 77, dtype=torch.int32, device=dev)
    ev.eval_positions_device(d_pos.data_ptr(), n, d_ps.data_ptr(), d_po.data_ptr(), None)
    with pytest.raises(F.FnnueError) as e:
        ev.check()
    assert e.value.name == "FNNUE_E_POSITION"
    ps, po = d_ps.cpu().numpy(), d_po.cpu().numpy()
    ok = np.ones(n, dtype=bool)
    ok[hole] = False
    assert ps[hole] == 0 and po[hole] == 0
    assert np.array_equal(ps[ok], ops[:n][ok]) and np.array_equal(po[ok], opo[:n][ok])
    assert_exact(ev, pos[:n], ops[:n], opo[:n])  # the context stays usable

"""The two-ply search of the Fairy-Stockfish variants on the device (ABI 3.10),
bit-exact: the second reduction with the variant ranks on hand-made arrays
against the rule in Python (tests/test_vsearch2.py); fnnue_vsearch2_children
per variant against fnnue_vsearch1 on the extended games, the rule over
fnnue_build_vchildren's arrays and the variant oracle on the pv's last
position; positions with known answers (confirmed on the host with
game_vchildren / game_end before they went in here); the independence of the
results from the scratch budget and the actor's piece cuts (fresh child
processes); the capacity protocol and FNNUE_E_ARCH; and the engine actor at two
variant plies, with 0 and 1 plies and chess batches left exactly as they were.

racingKings has no legal position for rank 3 (a child all of whose replies lose
at once): when white reaches rank 8 and black cannot follow, the game is over at
once (the child has NO_MOVES | VARIANT, rank 4); when black can, a reply draws.
Rank 3 rests on the hand-made arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from oracle.oracle import VariantOracleNet
from tests import test_vsearch2 as R
from tests.conftest import ROOT, net_bytes

pytestmark = pytest.mark.gpu

ZH, AT, KOTH, RK, TC = (N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL, N.VARIANT_RACINGKINGS,
                        N.VARIANT_THREECHECK)
VARIANTS = (ZH, AT, KOTH, RK, TC)
NAME = {ZH: "crazyhouse", AT: "atomic", KOTH: "kingOfTheHill", RK: "racingKings", TC: "threeCheck"}
CHESS_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
RK_START = "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1"
START = {ZH: ZH_START, AT: CHESS_START, KOTH: CHESS_START, RK: RK_START, TC: CHESS_START}
NORM = 361
WON = F.END_WON
DECIDED = F.END_CHECK | F.END_EXTINCT | F.END_VARIANT
MIN_RECORDS = 219 * 219

# the hand-made games of tests/test_gpu_vsearch1.py, and a threeCheck game ending on the third check
ZH_POCKETS = "r3k2r/8/8/8/8/8/8/R3K2R[PNBRQpnbrq] w KQkq - 0 1"      # 306 children
ZH_MATE = ("7k/6pp/8/8/8/8/8/K7[R] w - - 0 1", "R@e8")
ZH_BLOCK = ("7k/6pp/8/8/8/8/8/K7[Rr] w - - 0 1", "R@e8")
ATOMIC_WIN = "g1f3 e7e6 f3g5 f8e7 g5f7"                              # Nxf7 explodes the black king
AT_960 = "r4k1r/8/8/8/8/8/8/R4KR1 w GAha - 0 1"
KOTH_STEP = "8/8/3k4/8/8/3K4/8/8 w - - 0 1"
KOTH_END = "e2e4 a7a6 e1e2 a6a5 e2d3 a5a4 d3d4"
RK_CATCH = ("8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8")
RK_HOME = "8/K7/8/7k/8/8/8/8 w - - 0 1"
RK_ENDS = ["h2h3 d1c3 h3h4 c3d1 h4h5 d1c3 h5h6 c3d1 h6g7 d1c3 g7h8",
           "h2h3 a2a3 h3h4 a3a4 h4h5 a4a5 h5h6 a5a6 h6g7 a6b7 g7h8 b7a8"]
TC_THIRD = "e2e4 e7e5 d1h5 b8c6 h5f7 e8f7 f1c4 f7e8 c4f7"            # white checks on plies 5, 7 and 9
# positions with known answers
AT_BLUNDER = (CHESS_START, "g1f3 e7e6 f3g5")       # black: all but f7f6, f7f5, d8g5 allow Nxf7 (the king explodes)
AT_SAFE = {"f7f6", "f7f5", "d8g5"}
KOTH_ONE = ("8/8/4k3/8/8/8/8/R6K w - - 0 1", "")   # only a1a5 keeps the black king off d5 and e5
TC_LAST = (CHESS_START, "e2e4 e7e5 d1h5 b8c6 h5f7 e8f7 f1c4")  # black, checked twice: f7f6 / f7e7 avoid a third
TC_SAFE = {"f7f6", "f7e7"}
ZH_MATED = ("7k/6pp/8/8/2B5/3B4/1B6/K7[R] b - - 0 1", "")  # h6 / h5: a rook drop mates either way
ZH_AVOID = ("7k/p5pp/8/8/2B5/8/1B6/K7[R] b - - 0 1", "")   # a6, a5 and h5 allow a mating drop; h6 does not
HAND = {
    ZH: [(ZH_POCKETS, "P@e4 P@d5 e4d5 Q@e2"), ZH_MATE, ZH_BLOCK, ZH_MATED, ZH_AVOID],
    AT: [(CHESS_START, ATOMIC_WIN), (CHESS_START, ATOMIC_WIN.rsplit(" ", 1)[0]), (AT_960, "f1a1 a8a7"), (AT_960, "")],
    KOTH: [(KOTH_STEP, ""), (CHESS_START, KOTH_END), KOTH_ONE],
    RK: [RK_CATCH, (RK_HOME, ""), (RK_START, RK_ENDS[0]), (RK_START, RK_ENDS[1])],
    TC: [(CHESS_START, TC_THIRD), TC_LAST],
}
GAMES = {v: [(START[v], F.random_vgame(700 + 10 * v + i, v, START[v], 10)) for i in range(3)] + HAND[v]
         for v in VARIANTS}


def as_tuples(recs):
    return [tuple(int(r[n]) for n in recs.dtype.names) for r in recs]


def first_plies(games):
    out, g0 = [], 0
    for _, m in games:
        out.append(g0)
        g0 += len(m.split()) + 1
    return out


def net_of(v):
    """The crazyhouse net, or the atomic net's bytes: kingOfTheHill, racingKings and threeCheck share its format."""
    return F.synthesize_variant_net(5, 256, ZH) if v == ZH else F.synthesize_variant_net(6, 256, AT)


@pytest.fixture(scope="module")
def evs():
    """A crazyhouse and an atomic context; the atomic net also serves kingOfTheHill, racingKings and threeCheck."""
    made = {v: F.Evaluator(F.Net.from_bytes_variant(net_of(v), v), 0) for v in (ZH, AT)}
    yield made
    for e in made.values():
        e.close()


def serving(evs, v):
    return evs[ZH] if v == ZH else evs[AT]


@pytest.fixture(scope="module")
def searched(evs):
    """Per variant: vsearch2 of GAMES[v] with the children's records, and the level-1 arrays (computed once)."""
    out = {}
    for v in VARIANTS:
        ev = serving(evs, v)
        best2, off, kb, km = ev.vsearch2(v, GAMES[v], children=True)
        _, coff, moves, end = ev.build_vchildren(v, GAMES[v])
        for a in (best2, off, kb, km, coff, moves, end):
            a.setflags(write=False)
        out[v] = (best2, off, kb, km, coff, moves, end)
    return out


# ---- 1. the second reduction alone ----

def hand_made():
    """Groups of 0, 1, 2, 33, 64, 65, 219 and 307 records over every flag byte and kind, the table's rows, every
    adjacent pair of ranks in both orders, ties, a group cut by npos and one beyond it."""
    rng = np.random.default_rng(11)
    end, off, cb = [], [0], []
    kid = R.kid
    flags = [0, 0, 0, 0, F.END_CHECK, F.END_NO_MOVES, F.END_NO_MOVES | F.END_CHECK, F.END_NO_MOVES | F.END_EXTINCT,
             F.END_NO_MOVES | F.END_VARIANT, WON, WON | F.END_NO_MOVES | F.END_VARIANT, F.END_VARIANT]

    def group(fl, kids):
        assert len(kids) == max(len(fl) - 1, 0)
        end.extend(fl), cb.extend(kids)
        off.append(len(end))

    for size in (0, 1, 2, 33, 64, 65, 219, 307):
        kids, fl = [], [0] * min(size, 1)
        for c in range(max(size - 1, 0)):
            f = int(flags[rng.integers(0, len(flags))]) if size < 307 else int(flags[rng.integers(0, 4)])
            kind = F.BEST_NONE if f & F.END_NO_MOVES else \
                int(rng.choice([F.BEST_CP] * 7 + [F.BEST_MATE, F.BEST_LOST, F.BEST_NONE]))
            fl.append(f)
            kids.append(kid(kind, int(rng.integers(-30000, 30000)), int(rng.integers(0, 400)),
                            int(rng.integers(1, 307)), int(rng.integers(1, 4096)), int(rng.integers(-2**31, 2**31)),
                            int(rng.integers(-2**31, 2**31))))
        group(fl, kids)
    # every row of the table as an only child
    for f, b in ((WON, kid(value=5, ps=3, po=-4)), (F.END_NO_MOVES | F.END_CHECK, kid(F.BEST_NONE, ps=-2**31)),
                 (F.END_NO_MOVES | F.END_EXTINCT, kid(F.BEST_NONE)), (F.END_NO_MOVES | F.END_VARIANT, kid(F.BEST_NONE)),
                 (F.END_NO_MOVES, kid(F.BEST_NONE, ps=9, po=1)), (0, kid(F.BEST_LOST, best=4, move=9, ps=7, nodes=3)),
                 (0, kid(F.BEST_MATE, best=5, move=10)), (F.END_CHECK, kid(value=-31, best=6, move=11))):
        group([0, f], [b])
    # every adjacent pair of ranks in one group, in both orders
    ladder = [(WON, kid()), (0, kid(F.BEST_MATE)), (0, kid(value=2**28)), (0, kid(value=-2**28)),
              (0, kid(F.BEST_LOST)), (F.END_NO_MOVES | F.END_VARIANT, kid(F.BEST_NONE))]
    for lo in range(len(ladder) - 1):
        for pair in ((lo, lo + 1), (lo + 1, lo)):
            group([0] + [ladder[i][0] for i in pair], [ladder[i][1] for i in pair])
    group([0] * 41, [kid(value=-10, best=c + 1, nodes=3) for c in range(40)])             # a tie: the lowest index
    group([0] * 71, [kid(value=50)] * 69 + [kid(value=-50, best=4)])                      # the maximum at the last record
    group([0] * 71, [kid(F.BEST_MATE)] * 69 + [kid(F.BEST_LOST, best=4, move=8)])         # ... by rank
    group([2, WON, WON | F.END_NO_MOVES | F.END_VARIANT, F.END_NO_MOVES | F.END_VARIANT],
          [kid(ps=1), kid(F.BEST_NONE, ps=2), kid(F.BEST_NONE, ps=3)])                     # WON | NO_MOVES | VARIANT is lost
    group([1, WON, 0x4B, WON], [kid(ps=5, po=6, nodes=2), kid(ps=1), kid(ps=2)])           # all children WON: the first
    group([0, 0, 0, 0], [kid(F.BEST_MATE, nodes=4, best=3, move=5), kid(F.BEST_MATE, nodes=6), kid(F.BEST_MATE)])
    group([0, 0, 0], [kid(value=2**28), kid(value=-2**28)])                                # the value's whole range
    group([0, 0, 0], [kid(F.BEST_MATE), kid(value=2**28)])                                 # the worst value beats a mated
    group([0, 0, 0], [kid(value=-2**28), kid(F.BEST_LOST)])                                # the best value loses to rank 3
    group([0, 0, F.END_NO_MOVES, 0], [kid(value=3), kid(F.BEST_NONE, ps=40, po=-2**31), kid(value=0)])  # stalemate ties 0
    group([], [])
    group([F.END_NO_MOVES | F.END_VARIANT], [])
    n = len(end)
    group([0, 0, 0, WON, 0], [kid(value=1), kid(value=-4), kid(value=-9), kid(value=-99)])  # cut to 3 records by npos
    group([0, 0], [kid()])                                                                 # wholly beyond npos
    npos = n + 3
    kept = len(cb) - 3
    return (np.array(end[:npos], dtype=np.uint8), (np.arange(npos) * 73 % 4096 + 64).astype(np.uint16),
            np.array(off, dtype=np.uint32), np.array(cb[:kept], dtype=F.BEST_DTYPE))


def test_vbest_replies_on_hand_made_groups(evs):
    ev = evs[AT]
    end, moves, off, cb = hand_made()
    assert int(off[-1]) > len(end)
    want = R.vrule_over_groups(end, moves, off, as_tuples(cb))
    got = as_tuples(ev.vbest_replies(end, moves, off, cb))
    for g, (a, b) in enumerate(zip(got, want)):
        assert a == b, (g, dict(zip(F.BEST2_DTYPE.names, a)), dict(zip(F.BEST2_DTYPE.names, b)))
    assert len(got) == len(want) == len(off) - 1
    rec = lambda g: dict(zip(F.BEST2_DTYPE.names, got[g]))
    assert got[0] == (0,) * 12 and got[-1] == (0,) * 12 and rec(1)["kind"] == F.BEST_NONE
    assert {r[8] for r in got} == {F.BEST_NONE, F.BEST_CP, F.BEST_MATE, F.BEST_MATED, F.BEST_LOST}
    before = sum(max(s - 1, 0) for s in (0, 1, 2, 33, 64, 65, 219))
    assert rec(7)["nodes"] == 306 + int(cb["nodes"][before:before + 306].sum())
    rows = [rec(8 + i) for i in range(8)]
    assert [(r["kind"], r["pv_len"]) for r in rows] == \
        [(F.BEST_LOST, 1), (F.BEST_MATE, 1), (F.BEST_MATE, 1), (F.BEST_MATE, 1), (F.BEST_CP, 1), (F.BEST_MATE, 2),
         (F.BEST_MATED, 2), (F.BEST_CP, 2)]
    assert (rows[0]["psqt"], rows[0]["positional"], rows[0]["value"]) == (-3, 4, 0)
    assert rows[1]["psqt"] == -2**31                              # negated with wrap-around
    assert (rows[5]["reply_index"], rows[5]["reply"], rows[5]["psqt"], rows[5]["nodes"]) == (4, 9, 7, 4)
    assert (rows[7]["value"], rows[7]["reply_index"], rows[7]["reply"]) == (31, 6, 11)
    pairs = [rec(16 + i)["best"] for i in range(10)]
    assert pairs == [2, 1] * 5                                   # the higher rank wins in either order
    assert rec(26)["best"] == 1 and rec(27)["best"] == 70 and rec(28)["best"] == 70 and rec(28)["kind"] == F.BEST_MATE
    assert (rec(29)["best"], rec(29)["kind"], rec(29)["end"]) == (3, F.BEST_MATE, 2)
    assert (rec(30)["best"], rec(30)["kind"], rec(30)["psqt"], rec(30)["positional"], rec(30)["nodes"], rec(30)["end"]) == \
        (1, F.BEST_LOST, -5, -6, 5, 1)
    assert (rec(31)["kind"], rec(31)["best"], rec(31)["reply_index"], rec(31)["reply"], rec(31)["nodes"]) == \
        (F.BEST_MATED, 1, 3, 5, 13)
    assert (rec(32)["best"], rec(32)["value"]) == (2, 2**28) and (rec(33)["best"], rec(33)["value"]) == (2, -2**28)
    assert (rec(34)["best"], rec(34)["kind"], rec(34)["pv_len"]) == (2, F.BEST_MATE, 2)
    assert (rec(35)["best"], rec(35)["pv_len"], rec(35)["psqt"], rec(35)["positional"]) == (2, 1, -40, -2**31)
    assert got[36] == (0,) * 12 and got[37] == (0, 0, 0, 0, 0, 0, 0, 0, F.BEST_NONE, 9, 0, 0)
    assert (rec(38)["nodes"], rec(38)["best"], rec(38)["value"]) == (2, 2, 4)  # two of its four children are left
    # without a moves array: the same records, move 0
    bare = as_tuples(ev.vbest_replies(end, None, off, cb))
    assert bare == R.vrule_over_groups(end, None, off, as_tuples(cb)) and all(r[6] == 0 for r in bare)


def test_vbest_replies_equals_best_replies_on_chess_inputs(evs):
    from tests.test_gpu_search2 import hand_made as chess_hand_made
    ev = evs[ZH]
    end, moves, off, cb = chess_hand_made()
    assert int(end.max()) <= 3 and set(int(k) for k in cb["kind"]) <= {F.BEST_NONE, F.BEST_CP, F.BEST_MATE}
    assert ev.vbest_replies(end, moves, off, cb).tobytes() == ev.best_replies(end, moves, off, cb).tobytes()
    assert ev.vbest_replies(end, None, off, cb).tobytes() == ev.best_replies(end, None, off, cb).tobytes()


def test_vbest_replies_device_form_is_identical(evs):
    import torch
    ev = evs[AT]
    end, moves, off, cb = hand_made()
    want = ev.vbest_replies(end, moves, off, cb)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev)
    d_end, d_moves, d_off, d_cb = up(end), up(moves), up(off), up(cb)
    d_out = torch.full((len(want) * N.BEST2_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ev.vbest_replies_device(d_end.data_ptr(), d_moves.data_ptr(), d_off.data_ptr(), len(off) - 1, len(end),
                            d_cb.data_ptr(), d_out.data_ptr(), None)
    ev.check()
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST2_DTYPE), want)


# ---- 2. vsearch2 per variant ----

def test_games_are_what_they_should_be():
    assert F.game_end(CHESS_START, TC_THIRD, TC) == F.END_NO_MOVES | F.END_VARIANT | F.END_CHECK
    assert F.game_end(CHESS_START, ATOMIC_WIN, AT) & F.END_EXTINCT
    assert F.game_end(CHESS_START, KOTH_END, KOTH) == F.END_NO_MOVES | F.END_VARIANT
    for v in VARIANTS:
        assert all(len(m.split()) == 10 for _, m in GAMES[v][:3])


@pytest.mark.parametrize("v", VARIANTS)
def test_children_records_equal_vsearch1_on_extended_games(evs, searched, v):
    best2, off, kb, km, coff, moves, end = searched[v]
    ev = serving(evs, v)
    prefixes = [(fen, mv.split()[:q]) for fen, mv in GAMES[v] for q in range(len(mv.split()) + 1)]
    assert len(prefixes) == len(best2) == len(coff) - 1 and len(kb) == len(end) - len(best2)
    # child_map: (ply, 1-based child index) in record order
    want_map = [(p, c) for p in range(len(best2)) for c in range(1, int(coff[p + 1] - coff[p]))]
    assert [tuple(int(x) for x in m) for m in km] == want_map
    ext = [(prefixes[p][0], " ".join(prefixes[p][1] + [F.vmove_uci(int(moves[int(coff[p]) + c]))])) for p, c in want_map]
    best, goff = ev.vsearch1(v, ext)
    last = best[goff[1:] - 1]
    has_move = last["kind"] != F.BEST_NONE
    assert has_move.sum() > 300 and (~has_move).sum() >= 1
    assert np.array_equal(kb[has_move], last[has_move])
    for n in ("value", "nodes", "best", "move", "kind", "end"):  # a child without a legal move: its own terms, not zeros
        assert np.array_equal(kb[n][~has_move], last[n][~has_move])


@pytest.mark.parametrize("v", VARIANTS)
def test_vsearch2_equals_the_rule_over_the_children(evs, searched, v):
    best2, off, kb, km, coff, moves, end = searched[v]
    assert off.tolist() == np.cumsum([0] + [len(m.split()) + 1 for _, m in GAMES[v]]).tolist()
    want = R.vrule_over_groups(end, moves, coff, as_tuples(kb))
    got = as_tuples(best2)
    for p, (a, b) in enumerate(zip(got, want)):
        assert a == b, (p, dict(zip(F.BEST2_DTYPE.names, a)), dict(zip(F.BEST2_DTYPE.names, b)))
    assert len(got) == len(want)
    assert np.array_equal(serving(evs, v).vsearch2(v, GAMES[v])[0], best2)  # the plain host form
    kinds = {int(k) for k in best2["kind"]}
    assert {F.BEST_NONE, F.BEST_CP, F.BEST_MATE} <= kinds
    if v == ZH:
        first = first_plies(GAMES[v])
        assert int(coff[first[3] + 1] - coff[first[3]]) == 307  # the full-pocket ply: 306 children


@pytest.mark.parametrize("v", VARIANTS)
def test_pv_terms_equal_the_variant_oracle(searched, v):
    """The terms of the chosen pv's last position, replayed on the host, from the variant oracle (in the
    record's sign convention)."""
    best2 = searched[v][0]
    prefixes = [(fen, mv.split()[:q]) for fen, mv in GAMES[v] for q in range(len(mv.split()) + 1)]
    picked = [p for p in range(len(best2)) if best2[p]["kind"] == F.BEST_CP and best2[p]["pv_len"] == 2][:6]
    assert len(picked) >= 2
    recs = []
    for p in picked:
        fen, pre = prefixes[p]
        pv = [F.vmove_uci(int(best2[p]["move"])), F.vmove_uci(int(best2[p]["reply"]))]
        recs.append(F.game_vpositions(v, fen, pre + pv)[-1])
    # kingOfTheHill, racingKings and threeCheck: the feature set and the file format are atomic's
    ps, po = VariantOracleNet(net_of(v), ZH if v == ZH else AT).eval_packed(np.array(recs))[:2]
    # a two-move pv carries b_c's terms as they are, and fnnue_best negates its best child's: the record holds
    # the last position's terms negated with wrap-around, and its value is theirs from the ply's side to move
    assert [R.wrap_neg(x) for x in ps] == [int(best2[p]["psqt"]) for p in picked]
    assert [R.wrap_neg(x) for x in po] == [int(best2[p]["positional"]) for p in picked]
    for p, a, b in zip(picked, ps, po):
        s = int(a) + int(b)
        assert int(best2[p]["value"]) == abs(s) // 16 * (1 if s >= 0 else -1)


# ---- 3. positions with known answers ----

def ply_of(v, game, q):
    return first_plies(GAMES[v])[GAMES[v].index(game)] + q


def children_of(searched, v, p):
    """{move text: the child's depth-1 tuple} of ply p."""
    _, _, kb, _, coff, moves, _ = searched[v]
    o, e = int(coff[p]), int(coff[p + 1])
    kbt = as_tuples(kb[o - p:e - p - 1])
    return {F.vmove_uci(int(moves[o + c])): kbt[c - 1] for c in range(1, e - o)}


def test_atomic_two_plies_avoid_the_exploding_reply(evs, searched):
    p = ply_of(AT, (CHESS_START, ATOMIC_WIN), 3)
    kids = children_of(searched, AT, p)
    assert {t for t, b in kids.items() if b[6] != F.BEST_MATE} == AT_SAFE and len(kids) == 28
    one = serving(evs, AT).vsearch1(AT, [AT_BLUNDER])[0][-1]
    blunder = F.vmove_uci(int(one["move"]))
    assert one["kind"] == F.BEST_CP and blunder not in AT_SAFE  # at one ply: a move that lets the king explode
    assert F.vmove_uci(int(kids[blunder][5])) in ("g5f7", "g5e6")
    r = searched[AT][0][p]
    assert r["kind"] == F.BEST_CP and r["pv_len"] == 2 and F.vmove_uci(int(r["move"])) in AT_SAFE


def test_koth_only_one_move_keeps_the_king_off_the_hill(searched):
    p = ply_of(KOTH, KOTH_ONE, 0)
    kids = children_of(searched, KOTH, p)
    assert [t for t, b in kids.items() if b[6] != F.BEST_MATE] == ["a1a5"] and len(kids) == 16
    r = searched[KOTH][0][p]
    assert (r["kind"], r["pv_len"], F.vmove_uci(int(r["move"]))) == (F.BEST_CP, 2, "a1a5")
    # the step onto the hill itself: a mate in one, a one-move pv
    r = searched[KOTH][0][ply_of(KOTH, (KOTH_STEP, ""), 0)]
    assert (r["kind"], r["pv_len"], r["reply"]) == (F.BEST_MATE, 1, 0) and F.vmove_uci(int(r["move"])) in ("d3d4", "d3e4")


def test_threecheck_one_check_from_losing(searched):
    p = ply_of(TC, TC_LAST, 7)
    kids = children_of(searched, TC, p)
    assert {t for t, b in kids.items() if b[6] != F.BEST_MATE} == TC_SAFE and len(kids) == 5
    r = searched[TC][0][p]
    assert r["kind"] == F.BEST_CP and F.vmove_uci(int(r["move"])) in TC_SAFE
    # the game that went on with f7e8: white's third check is a mate in one
    r = searched[TC][0][ply_of(TC, (CHESS_START, TC_THIRD), 8)]
    assert (r["kind"], r["pv_len"], r["reply"]) == (F.BEST_MATE, 1, 0)
    last = searched[TC][0][ply_of(TC, (CHESS_START, TC_THIRD), 9)]
    assert last["kind"] == F.BEST_NONE and last["end"] == F.END_NO_MOVES | F.END_VARIANT | F.END_CHECK


def test_crazyhouse_mating_drop_as_the_reply(searched):
    r = searched[ZH][0][ply_of(ZH, ZH_MATED, 0)]
    assert (r["kind"], r["pv_len"], r["best"], F.vmove_uci(int(r["move"]))) == (F.BEST_MATED, 2, 1, "h7h6")
    assert F.vmove_uci(int(r["reply"])).startswith("R@")
    p = ply_of(ZH, ZH_AVOID, 0)
    kids = children_of(searched, ZH, p)
    assert [t for t, b in kids.items() if b[6] != F.BEST_MATE] == ["h7h6"] and len(kids) == 4
    r = searched[ZH][0][p]
    assert (r["kind"], r["pv_len"], F.vmove_uci(int(r["move"]))) == (F.BEST_CP, 2, "h7h6")
    r = searched[ZH][0][ply_of(ZH, ZH_MATE, 0)]  # the drop that mates at once: a one-move pv
    assert r["kind"] == F.BEST_MATE and r["pv_len"] == 1 and F.vmove_uci(int(r["move"])).startswith("R@")


def test_racingkings_reaching_rank_eight_is_not_a_win_while_black_can_follow(searched):
    p = ply_of(RK, RK_CATCH, 0)
    kids = children_of(searched, RK, p)
    for t in ("a7a8", "a7b8"):  # black follows and draws; its three other moves lose at once
        assert (kids[t][6], kids[t][2]) == (F.BEST_CP, 0) and F.vmove_uci(kids[t][5]) in ("h7g8", "h7h8")
    r = searched[RK][0][p]
    assert r["kind"] == F.BEST_CP and r["pv_len"] == 2
    if F.vmove_uci(int(r["move"])) in ("a7a8", "a7b8"):
        assert r["value"] == 0
    # with the black king out of reach the same move ends the game: a mate in one
    r = searched[RK][0][ply_of(RK, (RK_HOME, ""), 0)]
    assert (r["kind"], r["pv_len"], F.vmove_uci(int(r["move"]))) == (F.BEST_MATE, 1, "a7a8")


# ---- 4. the scratch budget ----

BUDGET_CHILD = """
import sys
import numpy as np
import fishnet_amd as F
from tests.test_gpu_vsearch2 import GAMES, VARIANTS, ZH, AT, net_of
evs = {v: F.Evaluator(F.Net.from_bytes_variant(net_of(v), v), 0) for v in (ZH, AT)}
out = [evs[ZH if v == ZH else AT].vsearch2(v, GAMES[v])[0] for v in VARIANTS]
np.save(sys.argv[1], np.concatenate(out))
"""


def test_results_do_not_depend_on_the_budget(searched, tmp_path):
    nodes = searched[ZH][0]["nodes"].astype(np.int64)
    assert nodes.max() > MIN_RECORDS  # the full-pocket ply's records alone exceed the smallest budget
    assert sum(int(searched[v][0]["nodes"].sum()) for v in VARIANTS) > 4 * MIN_RECORDS
    path = str(tmp_path / "small.npy")
    env = dict(os.environ, FNNUE_SEARCH2_RECORDS="1")  # forced up to its floor
    subprocess.run([sys.executable, "-c", BUDGET_CHILD, path], cwd=ROOT, env=env, check=True, timeout=300)
    small = np.load(path)
    assert small.dtype == F.BEST2_DTYPE
    assert small.tobytes() == np.concatenate([searched[v][0] for v in VARIANTS]).tobytes()


# ---- 5. the capacity protocol and FNNUE_E_ARCH ----

def test_vsearch2_device_form_and_capacity_protocol(evs, searched):
    import ctypes as C
    import torch
    v, ev = ZH, evs[ZH]
    out, off = searched[v][0], searched[v][1]
    dev = torch.device("cuda", 0)
    text, fen_off, mv_off = F.pack_games(GAMES[v])
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    ng = len(GAMES[v])
    d_off = torch.full((ng + 1,), -1, dtype=torch.int32, device=dev)
    d_out = torch.full((len(out) * N.BEST2_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    n, g = C.c_size_t(), C.c_size_t()
    args = (ev._h, v, C.c_void_p(d_text.data_ptr()), C.c_void_p(d_fo.data_ptr()), C.c_void_p(d_mo.data_ptr()), ng)
    for d, cap, o, ocap in ((None, 0, None, 0), (d_out.data_ptr(), len(out) - 1, d_off.data_ptr(), ng + 1),
                            (d_out.data_ptr(), len(out), d_off.data_ptr(), ng)):
        rc = N.lib.fnnue_vsearch2_device(*args, C.c_void_p(d), cap, C.c_void_p(o), ocap, C.byref(n), C.byref(g), None)
        assert rc == -10 and (n.value, g.value) == (len(out), ng)
    torch.cuda.synchronize(dev)
    assert bool((d_out == 0xAB).all()) and bool((d_off == -1).all())
    assert ev.vsearch2_device(v, d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, d_out.data_ptr(), len(out),
                              d_off.data_ptr(), ng + 1, None) == (len(out), ng)
    ev.check()
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST2_DTYPE), out)
    assert d_off.cpu().numpy().tolist() == off.tolist()
    # the children's count comes back with FNNUE_E_CAPACITY too
    k = C.c_size_t()
    best2 = np.zeros(len(out), dtype=F.BEST2_DTYPE)
    hoff = np.zeros(ng + 1, dtype=np.uint32)
    rc = N.lib.fnnue_vsearch2_children(ev._h, v, text, len(text), N.ptr(fen_off), N.ptr(mv_off), ng, N.ptr(best2),
                                       len(best2), N.ptr(hoff), len(hoff), None, None, 0, C.byref(n), C.byref(g),
                                       C.byref(k))
    assert rc == -10 and (n.value, g.value, k.value) == (len(out), ng, len(searched[v][2]))


def test_vsearch2_needs_the_variants_net_and_names_a_bad_move(evs):
    chess = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
    try:
        for v in (ZH, AT, 0):
            with pytest.raises(F.FnnueError) as err:
                chess.vsearch2(v, [(CHESS_START, "e2e4")])
            assert err.value.code == -4
    finally:
        chess.close()
    with pytest.raises(F.FnnueError) as err:
        evs[ZH].vsearch2(AT, [(CHESS_START, "e2e4")])
    assert err.value.code == -4
    with pytest.raises(F.FnnueError) as err:
        evs[ZH].vsearch2(KOTH, [(CHESS_START, "e2e4")])
    assert err.value.code == -4
    for v in (KOTH, RK, TC):  # the atomic net serves them
        assert len(evs[AT].vsearch2(v, [(START[v], "")])[0]) == 1
    with pytest.raises(F.FnnueError) as err:
        evs[AT].vsearch2(AT, [(CHESS_START, "e2e4"), (CHESS_START, "e2e4 e2e4")])
    assert err.value.code == -8 and "game 1" in str(err.value)


# ---- 6. the engine actor ----

def nets():
    kw = {NAME[v].lower(): F.Net.from_bytes_variant(net_of(v), v) for v in VARIANTS}
    return F.Net.from_bytes(net_bytes(1, 256, 0)), kw


@pytest.fixture(scope="module")
def chans():
    """(a channel at 2 variant plies, a set_variant_analysis_depth(1) channel, a channel never set): all six nets."""
    made = []
    for kw in ({"variant_analysis_plies": 2}, {"variant_analysis_depth": 1}, {}):
        chess, vnets = nets()
        made.append(B.channel(chess, 0, **vnets, **kw))
    yield tuple(stub for stub, _ in made)
    for _, actor in made:
        actor.close()


def bodies_of(v, games, **kw):
    return [B.AcquireResponseBody(f"{NAME[v]}{i}", fen, mv, variant=NAME[v], **kw) for i, (fen, mv) in enumerate(games)]


def strip(res, reply=True):
    out = []
    for rows in res:
        if isinstance(rows, B.PositionFailed):
            out.append(("failed", rows.code))
        else:
            out.append([(r.position_id, r.skipped, r.score and (r.score.kind, r.score.value), r.psqt, r.positional,
                         r.depth, r.nodes, r.best_move, r.matrix, r.reply if reply else None) for r in rows])
    return out


def trunc_div(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)


def check_two_plies(rows, zero_rows, recs):
    assert len(rows) == len(recs)
    for q, (r, z, b) in enumerate(zip(rows, zero_rows, recs)):
        assert r.position_id == q
        if b["kind"] == F.BEST_NONE:  # exactly as on a never-set channel
            assert (z.depth, z.nodes, z.best_move) == (0, 0, None)
            assert (r.score, r.depth, r.nodes, r.best_move, r.reply, r.psqt, r.positional) == \
                (B.Score("mate" if b["end"] & DECIDED else "cp", 0), 0, 0, None, None, z.psqt, z.positional)
            continue
        score = {F.BEST_MATE: B.Score("mate", 1), F.BEST_MATED: B.Score("mate", -1),
                 F.BEST_LOST: B.Score("mate", -1)}.get(int(b["kind"]),
                                                       B.Score("cp", trunc_div(int(b["value"]) * 100, NORM)))
        assert (r.score, r.depth, r.nodes, r.best_move, r.reply, r.psqt, r.positional) == \
            (score, int(b["pv_len"]), int(b["nodes"]), F.vmove_uci(int(b["move"])),
             F.vmove_uci(int(b["reply"])) or None, int(b["psqt"]), int(b["positional"]))


def actor_context_records(v):
    """vsearch2 of GAMES[v] on a context of the net the actor uses for v (the same bytes loaded as v's own net,
    where `searched` evaluates kingOfTheHill, racingKings and threeCheck on the atomic net's context)."""
    ev = F.Evaluator(F.Net.from_bytes_variant(net_of(v), v), 0)
    try:
        return ev.vsearch2(v, GAMES[v])
    finally:
        ev.close()


@pytest.mark.parametrize("v", VARIANTS)
def test_actor_two_plies_against_vsearch2(chans, searched, v):
    d2, _, d0 = chans
    out, off = (searched[v][0], searched[v][1]) if v in (ZH, AT) else actor_context_records(v)
    bodies = bodies_of(v, GAMES[v])
    res, zero = d2.go_pv(bodies), d0.go(bodies)
    for i, (rows, zrows) in enumerate(zip(res, zero)):
        assert not isinstance(rows, B.PositionFailed), rows
        check_two_plies(rows, zrows, out[off[i]:off[i + 1]])
    assert B.last_stats(d2._actor)["positions"] == len(out) + int(out["nodes"].sum())  # plies + children + grandchildren
    plain = d2.go(bodies)  # go(): the same responses without the reply
    assert all(r.reply is None for rows in plain for r in rows) and strip(plain) == strip(res, reply=False)
    # the JSON carries the reply
    rows = res[0]
    parts = json.loads(B.into_analysis(rows))
    for r, part in zip(rows, parts):
        if r.reply:
            assert part["pv"] == r.best_move + " " + r.reply and part["depth"] == 2
    assert any(r.reply for r in rows)


def test_actor_json_with_a_drop_in_the_pv(chans):
    d2 = chans[0]
    rows = d2.go_pv(bodies_of(ZH, [ZH_MATED, ZH_BLOCK]))
    part = json.loads(B.into_analysis(rows[0]))[0]
    assert part["pv"].startswith("h7h6 R@") and part["score"] == {"mate": -1} and part["depth"] == 2
    block = json.loads(B.into_analysis(rows[1]))[1]  # after R@e8 black must block with a drop
    assert block["pv"].split()[0] in ("R@f8", "R@g8") and block["depth"] == 2


def test_actor_back_to_one_ply_and_zero_and_chess_unchanged(chans):
    d2, d1, d0 = chans
    from tests.test_search2 import GAMES as CHESS_GAMES
    chess = [B.AcquireResponseBody(f"c{i}", fen, mv, variant="fromPosition") for i, (fen, mv) in
             enumerate(CHESS_GAMES[5:8])]
    move = [B.AcquireResponseBody("mv", ZH_START, "e2e4 e7e5", work="move", variant="crazyhouse")]
    vb = bodies_of(ZH, GAMES[ZH][:2] + GAMES[ZH][4:]) + bodies_of(RK, GAMES[RK][3:5])
    try:
        # a chess batch and move work: the same at 0, 1 and 2 variant plies
        assert strip(d2.go_pv(chess)) == strip(d1.go(chess)) == strip(d0.go(chess))
        assert strip(d2.go_pv(move)) == strip(d1.go(move)) == strip(d0.go(move))
        lines2, lines1 = (d.go_lines(bodies_of(ZH, GAMES[ZH][4:6], multipv=2)) for d in (d2, d1))  # a one-ply search
        assert strip(lines2) == strip(lines1) and lines2[0][0].depth == 1 and len(lines2[0][0].lines) == 2
        assert [[r.lines for r in rows] for rows in lines2] == [[r.lines for r in rows] for rows in lines1]
        d2.set_variant_analysis_plies(0)
        assert strip(d2.go_pv(vb)) == strip(d0.go(vb))
        d2.set_variant_analysis_plies(1)
        assert strip(d2.go_pv(vb)) == strip(d1.go(vb))
        for bad in (3, -1):
            with pytest.raises(F.FnnueError) as err:
                d2.set_variant_analysis_plies(bad)
            assert err.value.code == -1
        with pytest.raises(F.FnnueError) as err:
            d2.set_variant_analysis_depth(2)
        assert err.value.code == -1
        assert strip(d2.go_pv(vb)) == strip(d1.go(vb))  # a refused setter changes nothing
        d2.set_analysis_plies(2)                         # the chess setting is another field
        assert strip(d2.go_pv(vb)) == strip(d1.go(vb)) and d2.go_pv(chess)[0][0].depth == 2
        d2.set_analysis_plies(0)
        d2.set_variant_analysis_plies(2)
        assert strip(d2.go_pv(chess)) == strip(d0.go(chess))  # ... and the variant setter does not move it
    finally:
        d2.set_analysis_plies(0)
        d2.set_variant_analysis_plies(2)
    assert d2.go_pv(vb[:1])[0][0].depth == 2


def test_actor_failures_stay_isolated(chans):
    d2 = chans[0]
    good = bodies_of(AT, GAMES[AT][:2])
    mixed = [good[0], B.AcquireResponseBody("bad", CHESS_START, "e2e4 e7e5 e1e3", variant="atomic"), good[1]]
    res, alone = d2.go_pv(mixed), d2.go_pv(good)
    assert isinstance(res[1], B.PositionFailed) and res[1].code == -8
    assert strip([res[0], res[2]]) == strip(alone) and alone[0][0].depth == 2 and alone[0][0].reply


PIECES_CHILD = """
import json
from fishnet_amd import backend as B
from tests.test_gpu_vsearch2 import GAMES, VARIANTS, bodies_of, nets, strip
chess, vnets = nets()
stub, actor = B.channel(chess, 0, **vnets, variant_analysis_plies=2)
res = stub.go_pv([b for v in VARIANTS for b in bodies_of(v, GAMES[v])])
print("RESULT " + json.dumps({"rows": strip(res), "stats": B.last_stats(actor)}))
actor.close()
"""


def test_piece_cuts_do_not_change_the_answers(chans):
    d2 = chans[0]
    res = d2.go_pv([b for v in VARIANTS for b in bodies_of(v, GAMES[v])])
    stats = B.last_stats(d2._actor)
    assert stats["pieces"] == len(VARIANTS)
    env = dict(os.environ, FNNUE_BACKEND_PIECE_PLIES="1")  # forced up to its minimum: pieces of 16 plies
    out = subprocess.run([sys.executable, "-c", PIECES_CHILD], cwd=ROOT, env=env, check=True, capture_output=True,
                         text=True, timeout=300).stdout
    small = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert small["rows"] == json.loads(json.dumps(strip(res)))
    assert small["stats"]["pieces"] > stats["pieces"]
    plies = sum(len(rows) for rows in res)
    assert small["stats"]["positions"] == stats["positions"] == plies + sum(r.nodes for rows in res for r in rows)

"""The one-ply search on the device (ABI 3.4), bit-exact: the children
expansion with each record's move and end flags against host replays, the
STAR-group reduction on hand-made arrays against a dozen lines of Python,
fnnue_search1 against the oracle's evaluation of the host builder's records
reduced by that Python, and the engine actor at analysis depth 1 (best move,
pv, score, nodes; [ref] AnalysisPart::Best, src/api.rs:359-369) with depth 0
left exactly as it was."""
import json
import os

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from oracle.oracle import OracleNet
from tests.conftest import ROOT, net_bytes
from tests.positions import CHESS960, START

pytestmark = pytest.mark.gpu

WCC = json.load(open(os.path.join(ROOT, "tests", "golden", "wcc_games.json")))["games"]
MANY = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"  # 218 legal moves
FOOLS_MATE = "f2f3 e7e5 g2g4 d8h4"
STALEMATE = ("7k/5Q2/5K2/8/8/8/8/8 w - - 0 1", "f6g6")
MATE_OR_STALEMATE = "7k/5Q2/5K2/8/8/8/8/8 w - - 0 1"  # Qg7 / Qf8 mate, Kg6 stalemates
C960_MOVES = F.random_game(15, CHESS960, 30)          # its 7th move, g1h1, castles (king takes rook)
NORM = 361

GAMES = [(g["position"], " ".join(g["moves"].split()[:40])) for g in WCC[:6]]
GAMES += [(CHESS960, C960_MOVES), (MANY, "")]
SEARCH_GAMES = GAMES + [(START, "f2f3 e7e5 g2g4"), (MATE_OR_STALEMATE, ""), (START, FOOLS_MATE), STALEMATE]


def wrap_neg(x):
    return ((-int(x) + 2**31) % 2**32) - 2**31


def reduce_groups(ps, po, end, moves, off):
    """fnnue_best_children in Python: (psqt, positional, value, nodes, best, move, kind, end) per group."""
    out = []
    for o, e in zip(off[:-1], off[1:]):
        o, e = int(o), int(e)
        if o == e:
            out.append((0,) * 8)
            continue
        best, key = 0, None
        for c in range(1, e - o):
            f = int(end[o + c])
            if f & F.END_NO_MOVES:
                k = (2, 0) if f & F.END_CHECK else (1, 0)
            else:
                s = int(ps[o + c]) + int(po[o + c])
                k = (1, -(abs(s) // 16 * (1 if s >= 0 else -1)))  # C truncation
            if key is None or k > key:  # the first maximum
                best, key = c, k
        if not best:
            out.append((0, 0, 0, e - o - 1, 0, 0, F.BEST_NONE, int(end[o])))
            continue
        kind = F.BEST_MATE if key[0] == 2 else F.BEST_CP
        out.append((wrap_neg(ps[o + best]), wrap_neg(po[o + best]), key[1] if kind == F.BEST_CP else 0, e - o - 1, best,
                    int(moves[o + best]) if moves is not None else 0, kind, int(end[o])))
    return out


def as_tuples(best):
    return [tuple(int(r[n]) for n in F.BEST_DTYPE.names) for r in best]


@pytest.fixture(scope="module")
def data():
    return net_bytes(1, 256, 0)


@pytest.fixture(scope="module")
def ev(data):
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kids(ev):
    """The device's children of SEARCH_GAMES (computed once, never changed)."""
    pos, off, moves, end = ev.build_children(SEARCH_GAMES)
    for a in (pos, off, moves, end):
        a.setflags(write=False)
    first, g0 = [], 0  # first group of each game
    for _, m in SEARCH_GAMES:
        first.append(g0)
        g0 += len(m.split()) + 1
    assert g0 == len(off) - 1
    return pos, off, moves, end, first


def test_c960_game_castles():
    ms = C960_MOVES.split()
    assert len(ms) == 30 and ms[6] == "g1h1"
    before, after = F.game_positions(CHESS960, ms[:7])[-2:]
    sq = lambda p, s: (int(p[s >> 1]) >> (4 * (s & 1))) & 15
    assert (sq(before, 6), sq(before, 7)) == (6, 4)                      # white king g1, rook h1
    assert (sq(after, 5), sq(after, 6), sq(after, 7)) == (4, 6, 0)       # rook f1, king g1


def test_children_records_and_offsets(kids):
    pos, off, _, _, first = kids
    for (fen, moves), g0 in zip(SEARCH_GAMES, first):
        hp, ho = F.game_children(fen, moves)
        n = len(ho) - 1
        assert np.array_equal(off[g0:g0 + n + 1] - off[g0], ho)
        assert np.array_equal(pos[off[g0]:off[g0 + n]], hp)
    assert int(off[first[7] + 1] - off[first[7]]) == 219


def test_children_equal_plain_builder(ev, kids):
    pos, off, _, _, _ = kids
    p2, o2 = ev.build_batch(SEARCH_GAMES, F.PLAYOUT_CHILDREN)
    assert np.array_equal(pos, p2) and np.array_equal(off, o2)


def test_children_moves_and_end_flags(kids):
    """Each child's move text replayed after the game's prefix gives exactly
    that record; each record's flags are the host's for the same prefix."""
    pos, off, moves, end, first = kids
    replays = 0
    for (fen, mv), g0 in zip(GAMES, first):
        ms = mv.split()
        for q in range(len(ms) + 1):
            o, e = int(off[g0 + q]), int(off[g0 + q + 1])
            prefix = ms[:q]
            assert moves[o] == 0
            assert end[o] == F.game_end(fen, prefix), (fen, prefix)
            assert bool(end[o] & F.END_NO_MOVES) == (e - o == 1)
            texts = [F.move_uci(int(m)) for m in moves[o + 1:e]]
            assert len(set(texts)) == len(texts)
            for x, t in zip(range(o + 1, e), texts):
                assert np.array_equal(F.game_positions(fen, prefix + [t])[-1], pos[x]), (fen, prefix, t)
                assert end[x] == F.game_end(fen, prefix + [t]), (fen, prefix, t)
                replays += 1
            if q < len(ms):
                assert ms[q] in texts  # the game's own notation
    assert replays > 5000
    assert "g1h1" in [F.move_uci(int(m)) for m in moves[off[first[6] + 6] + 1:off[first[6] + 7]]]


def hand_made_groups():
    """Group sizes 0, 1, 2, 33, 64, 65 and 219 in one call, then the special cases."""
    rng = np.random.default_rng(5)
    ps, po, end, off = [], [], [], [0]

    def group(p, q, f):
        ps.extend(p), po.extend(q), end.extend(f)
        off.append(len(ps))

    for size in (0, 1, 2, 33, 64, 65, 219):
        group(rng.integers(-40000, 40000, size), rng.integers(-40000, 40000, size), [0] * size)
    group([0] + [160] * 40, [0] + [-320] * 40, [0] * 41)                     # equal values: the lowest index wins
    group([5, -16 * 10**6, 7, 9], [0, 0, 0, 0], [0, 0, 0, 3])                # a mate behind a child worth +10^6
    group([0, 100, 900, 16, 40], [0, 60, 0, 16, 0], [0, 0, 0, 1, 0])         # a stalemate among negative children
    group([0, 17, 1, -17, 1], [0, 0, 0, 0, 0], [0] * 5)                      # -17 / 16 = -1, 17 / 16 = 1: truncation
    group([0, 31, -31], [0, 0, 0], [0] * 3)                                  # +-31 / 16 = +-1
    group([0, 2**31 - 1, 0], [0, 2**31 - 1, 0], [2, 0, 0])                   # the 64-bit sum, both ways
    group([0, 0, -2**31], [0, 0, -2**31], [0, 0, 0])
    group([0, 2**31 - 1, 2**31 - 1], [0, -2**31, -2**31 + 16], [0, 0, 0])
    group([3] + [50] * 69 + [-50], [0] * 71, [0] * 71)                       # the maximum at the last record
    group([0, 0, 0, 0], [0, 0, 0, 0], [0, 3, 3, 1])                          # two mates: the first
    group([], [], [])                                                        # an empty group at the end
    n = len(ps)
    return (np.array(ps, dtype=np.int64).astype(np.int32), np.array(po, dtype=np.int64).astype(np.int32),
            np.array(end, dtype=np.uint8), (np.arange(n) * 73 % 4096 + 64).astype(np.uint16),
            np.array(off, dtype=np.uint32))


def test_reduction_on_hand_made_groups(ev):
    ps, po, end, moves, off = hand_made_groups()
    want = reduce_groups(ps, po, end, moves, off)
    got = as_tuples(ev.best_children(ps, po, end, moves, off))
    assert got == want
    names = F.BEST_DTYPE.names
    rec = lambda g: dict(zip(names, got[g]))
    assert got[0] == (0,) * 8 and got[-1] == (0,) * 8
    assert rec(1)["kind"] == F.BEST_NONE and rec(1)["nodes"] == 0
    assert rec(7)["best"] == 1 and rec(7)["value"] == 10
    assert rec(8)["kind"] == F.BEST_MATE and rec(8)["best"] == 3 and rec(8)["value"] == 0
    assert rec(9)["best"] == 3 and rec(9)["value"] == 0 and rec(9)["kind"] == F.BEST_CP
    assert rec(10)["best"] == 3 and rec(10)["value"] == 1
    assert rec(11)["best"] == 2 and rec(11)["value"] == 1
    assert rec(12)["best"] == 2 and rec(12)["value"] == 0 and rec(12)["end"] == 2
    assert rec(13)["best"] == 2 and rec(13)["value"] == 2**28 and rec(13)["psqt"] == -2**31
    assert rec(14)["best"] == 1 and rec(14)["value"] == 0
    assert rec(15)["best"] == 70 and rec(15)["value"] == 3
    assert rec(16)["best"] == 1 and rec(16)["kind"] == F.BEST_MATE
    # without a moves array: the same records, move 0
    bare = as_tuples(ev.best_children(ps, po, end, None, off))
    assert bare == reduce_groups(ps, po, end, None, off)


@pytest.fixture(scope="module")
def searched(ev, data, kids):
    """search1 of SEARCH_GAMES and what it must be: the oracle's evaluation of
    the host builder's records, reduced in Python with the host's end flags."""
    pos, off, moves, end, first = kids
    ops, opo, rc = OracleNet(data).eval_packed(pos, threads=8)
    assert rc == 0
    hend = np.array(end)  # GAMES' flags are checked against the host above; the short games' here
    for (fen, mv), g0 in list(zip(SEARCH_GAMES, first))[len(GAMES):]:
        ms = mv.split()
        for q in range(len(ms) + 1):
            o, e = int(off[g0 + q]), int(off[g0 + q + 1])
            hend[o] = F.game_end(fen, ms[:q])
            for x in range(o + 1, e):
                hend[x] = F.game_end(fen, ms[:q] + [F.move_uci(int(moves[x]))])
    want = reduce_groups(ops, opo, hend, moves, off)
    best, goff = ev.search1(SEARCH_GAMES)
    best.setflags(write=False)
    return best, goff, want, first


def test_search1_matches_oracle_restatement(searched):
    best, goff, want, first = searched
    assert goff.tolist() == first + [len(want)]
    assert as_tuples(best) == want
    for r in best[: goff[8]]:  # the games: every ply has a legal best move
        assert r["kind"] != F.BEST_NONE and r["move"] != 0 and 1 <= r["best"] <= r["nodes"]


def test_search1_mates_and_terminal_roots(searched):
    best, goff, _, _ = searched
    r = best[goff[8] + 3]  # after f2f3 e7e5 g2g4
    assert (r["kind"], F.move_uci(int(r["move"])), r["value"], r["end"]) == (F.BEST_MATE, "d8h4", 0, 0)
    r = best[goff[9]]      # mating and stalemating children together: the first mate in generation order
    assert r["kind"] == F.BEST_MATE and F.move_uci(int(r["move"])) in ("f7g7", "f7f8") and r["nodes"] > 20
    r = best[goff[11] - 1]  # fool's mate played out
    assert tuple(int(r[n]) for n in F.BEST_DTYPE.names) == (0, 0, 0, 0, 0, 0, F.BEST_NONE,
                                                             F.END_NO_MOVES | F.END_CHECK)
    r = best[goff[12] - 1]  # the stalemate
    assert (r["kind"], r["end"], r["nodes"], r["best"]) == (F.BEST_NONE, F.END_NO_MOVES, 0, 0)


def test_search1_device_form_is_identical(ev, searched):
    import torch
    best, goff, _, _ = searched
    dev = torch.device("cuda", 0)
    text, fen_off, mv_off = F.pack_games(SEARCH_GAMES)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    ng = len(SEARCH_GAMES)
    d_off = torch.zeros(ng + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(F.FnnueError) as err:  # too small: the sizes come back
        ev.search1_device(d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, 0, 0, d_off.data_ptr(), ng + 1, None)
    assert err.value.code == -10
    d_out = torch.zeros(len(best) * N.BEST_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    n, g = ev.search1_device(d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, d_out.data_ptr(), len(best),
                             d_off.data_ptr(), ng + 1, None)
    ev.check()
    assert (n, g) == (len(best), ng)
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST_DTYPE), best)
    assert d_off.cpu().numpy().tolist() == goff.tolist()


def test_search1_bad_move_is_named(ev):
    with pytest.raises(F.FnnueError) as err:
        ev.search1([(START, "e2e4"), (START, "e2e4 e2e4")])
    assert err.value.code == -8 and "game 1" in str(err.value)


# ---- the engine actor ----

ZH = N.VARIANT_CRAZYHOUSE
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
CROWDED = "rnbqkbnr/pppppppp/pppppppp/8/8/PPPPPPPP/PPPPPPPP/RNBQKBNR w - - 0 1"  # 48 pieces: replays, cannot be evaluated


@pytest.fixture(scope="module")
def chans(data):
    """(a depth-1 channel, a channel never set), both with a crazyhouse net."""
    zh = F.synthesize_variant_net(5, 256, ZH)
    made = []
    for depth in (1, 0):
        kw = {"analysis_depth": 1} if depth else {}
        made.append(B.channel(F.Net.from_bytes(data), 0, crazyhouse=F.Net.from_bytes_variant(zh, ZH), **kw))
    yield made[0][0], made[1][0]
    for _, actor in made:
        actor.close()


def bodies_of(games, **kw):
    return [B.AcquireResponseBody(f"g{i}", fen, mv, variant="chess960" if fen == CHESS960 else "fromPosition", **kw)
            for i, (fen, mv) in enumerate(games)]


def strip(res):
    """Every field but time_ms / nps."""
    out = []
    for rows in res:
        if isinstance(rows, B.PositionFailed):
            out.append(("failed", rows.code))
        else:
            out.append([(r.position_id, r.skipped, r.score and (r.score.kind, r.score.value), r.psqt, r.positional,
                         r.depth, r.nodes, r.best_move, r.matrix) for r in rows])
    return out


def trunc_div(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)


def check_depth1(rows, zero_rows, best):
    assert len(rows) == len(best)
    for q, (r, z, b) in enumerate(zip(rows, zero_rows, best)):
        assert r.position_id == q
        if b["kind"] == F.BEST_NONE:  # exactly as at depth 0
            assert (z.depth, z.nodes, z.best_move) == (0, 0, None)
            assert (r.score, r.depth, r.nodes, r.best_move, r.psqt, r.positional) == \
                (B.Score("mate" if b["end"] & F.END_CHECK else "cp", 0), 0, 0, None, z.psqt, z.positional)
            continue
        score = B.Score("mate", 1) if b["kind"] == F.BEST_MATE else B.Score("cp", trunc_div(int(b["value"]) * 100, NORM))
        assert (r.score, r.depth, r.nodes, r.best_move, r.psqt, r.positional) == \
            (score, 1, int(b["nodes"]), F.move_uci(int(b["move"])), int(b["psqt"]), int(b["positional"]))


def test_actor_depth1_against_search1(chans, searched):
    d1, d0 = chans
    best, goff, _, _ = searched
    bodies = bodies_of(SEARCH_GAMES)
    res, zero = d1.go(bodies), d0.go(bodies)
    children = 0
    for i, (rows, zrows) in enumerate(zip(res, zero)):
        assert not isinstance(rows, B.PositionFailed), rows
        check_depth1(rows, zrows, best[goff[i]:goff[i + 1]])
        children += sum(r.nodes for r in rows)
    assert B.last_stats(d1._actor)["positions"] == len(best) + children  # plies plus children
    assert strip(d1.go(bodies)) == strip(res)  # the same go() twice
    parts = json.loads(B.into_analysis(res[8]))
    assert parts[3]["pv"] == "d8h4" and parts[3]["score"] == {"mate": 1} and parts[0]["depth"] == 1
    last = json.loads(B.into_analysis(res[10]))[-1]
    assert "pv" not in last and last["score"] == {"mate": 0} and last["depth"] == 0


def test_actor_skipped_and_multipv(chans, searched):
    d1, _ = chans
    best, goff, _, _ = searched
    fen, mv = SEARCH_GAMES[8]
    rows = d1.go([B.AcquireResponseBody("s", fen, mv, skip_positions=[1, 3])])[0]
    assert [r.skipped for r in rows] == [False, True, False, True]
    assert rows[0].best_move == F.move_uci(int(best[goff[8]]["move"])) and rows[2].depth == 1
    rows = d1.go([B.AcquireResponseBody("m", fen, mv, multipv=1)])[0]
    parts = json.loads(B.into_analysis(rows))
    assert parts[3] == {"pv": [[None, ["d8h4"]]], "score": [[None, {"mate": 1}]], "depth": 1,
                        "nodes": int(best[goff[8] + 3]["nodes"]), "time": rows[3].time_ms,
                        **({"nps": rows[3].nps} if rows[3].nps else {})}
    assert B.into_analysis(rows[:1]).startswith('[{"pv":[[null,["' + rows[0].best_move + '"]]],"score":[[null,{"cp":')


def test_actor_failures_stay_isolated(chans, data):
    d1, d0 = chans
    good = bodies_of(SEARCH_GAMES[:2])
    zh_moves = F.random_vgame(1000, ZH, ZH_START, 30)
    mixed = [good[0], B.AcquireResponseBody("bad", START, "e2e4 e7e5 e1e3"), good[1],
             B.AcquireResponseBody("zh", ZH_START, zh_moves, variant="crazyhouse"),
             B.AcquireResponseBody("crowded", CROWDED, "a3a4", variant="fromPosition")]
    # a chess-only channel: the bad batch fails alone, the crazyhouse one has no net
    stub, actor = B.channel(F.Net.from_bytes(data), 0, analysis_depth=1)
    try:
        res = stub.go(mixed)
        alone = stub.go(good)
    finally:
        actor.close()
    assert isinstance(res[1], B.PositionFailed) and res[1].code == -8
    assert isinstance(res[3], B.PositionFailed) and res[3].code == -4
    assert isinstance(res[4], B.PositionFailed) and res[4].code == -6  # the evaluator rejects its positions
    assert strip([res[0], res[2]]) == strip(alone) and alone[0][0].depth == 1
    # with the net: the crazyhouse batch at depth 0, exactly as a depth-0 channel answers it
    res1, res0 = d1.go(mixed), d0.go(mixed)
    assert isinstance(res1[1], B.PositionFailed) and res1[1].code == -8
    assert isinstance(res1[4], B.PositionFailed) and res1[4].code == -6
    assert strip(res1[3:]) == strip(res0[3:]) and res1[3][0].depth == 0 and res1[3][0].nodes == 1
    assert strip([res1[0], res1[2]]) == strip(alone)


def test_actor_depth_back_to_zero(chans):
    d1, d0 = chans
    bodies = bodies_of(SEARCH_GAMES) + [B.AcquireResponseBody("mv", START, "e2e4 e7e5", work="move")]
    try:
        d1.set_analysis_depth(0)
        assert strip(d1.go(bodies)) == strip(d0.go(bodies))
    finally:
        d1.set_analysis_depth(1)
    with pytest.raises(F.FnnueError) as err:
        d1.set_analysis_depth(2)
    assert err.value.code == -1
    # move work is the same at either depth
    assert strip(d1.go(bodies[-1:])) == strip(d0.go(bodies[-1:]))


def test_actor_compact_form(chans):
    d1, _ = chans
    bodies = bodies_of(SEARCH_GAMES[6:], multipv=None)
    full, compact = d1.go(bodies), d1.go_compact(bodies)
    for rows, crows in zip(full, compact):
        assert [(r.score, r.depth, r.psqt, r.positional) for r in rows] == \
            [(r.score, r.depth, r.psqt, r.positional) for r in crows]
        assert all(r.best_move is None for r in crows)  # the 16-byte record has no room for a move

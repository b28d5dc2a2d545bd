"""The one-ply search of the Fairy-Stockfish variants on the device (ABI 3.6),
bit-exact: the variant children expansion with each record's move (drops as
"N@f3") and end flags (explosions, the variants' own game ends, the
racingKings child that fails to catch up) against host replays; the reduction's
variant ranks against a restatement of the rule in Python; fnnue_vsearch1 and
fnnue_vsearch1_lines against their three steps done one by one; and the engine
actor at variant analysis depth 1 against the project's own move work, with
depth 0 left exactly as it was."""
import json

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from tests.conftest import net_bytes

pytestmark = pytest.mark.gpu

ZH, AT, KOTH, RK = N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL, N.VARIANT_RACINGKINGS
VARIANTS = (ZH, AT, KOTH, RK)
NAME = {0: "standard", ZH: "crazyhouse", AT: "atomic", KOTH: "kingOfTheHill", RK: "racingKings"}
CHESS_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
RK_START = "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1"
START = {ZH: ZH_START, AT: CHESS_START, KOTH: CHESS_START, RK: RK_START}
NORM = 361
WON = F.END_WON
DECIDED = F.END_CHECK | F.END_EXTINCT | F.END_VARIANT

# hand-made games
ZH_POCKETS = "r3k2r/8/8/8/8/8/8/R3K2R[PNBRQpnbrq] w KQkq - 0 1"      # drops of every type; no pawn on ranks 1 and 8
ZH_MATE = ("7k/6pp/8/8/8/8/8/K7[R] w - - 0 1", "R@e8")               # a mate no drop can block
ZH_BLOCK = ("7k/6pp/8/8/8/8/8/K7[Rr] w - - 0 1", "R@e8")             # its twin: r@f8 / r@g8 block
ATOMIC_WIN = "g1f3 e7e6 f3g5 f8e7 g5f7"                              # Nxf7 explodes the black king
AT_960 = "r4k1r/8/8/8/8/8/8/R4KR1 w GAha - 0 1"                      # Chess960 castling: f1g1 and f1a1 take the rook
KOTH_STEP = "8/8/3k4/8/8/3K4/8/8 w - - 0 1"                          # d3d4 / d3e4 step onto the hill
KOTH_END = "e2e4 a7a6 e1e2 a6a5 e2d3 a5a4 d3d4"
RK_CATCH = ("8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8")                   # black must catch up: three moves lose at once
RK_HOME = "8/K7/8/7k/8/8/8/8 w - - 0 1"
RK_ENDS = ["h2h3 d1c3 h3h4 c3d1 h4h5 d1c3 h5h6 c3d1 h6g7 d1c3 g7h8",
           "h2h3 a2a3 h3h4 a3a4 h4h5 a4a5 h5h6 a5a6 h6g7 a6b7 g7h8 b7a8"]
HAND = {
    ZH: [(ZH_POCKETS, "P@e4 P@d5 e4d5 Q@e2"), ZH_MATE, ZH_BLOCK],
    AT: [(CHESS_START, ATOMIC_WIN), (CHESS_START, ATOMIC_WIN.rsplit(" ", 1)[0]), (AT_960, "f1a1 a8a7"), (AT_960, "")],
    KOTH: [(KOTH_STEP, ""), (CHESS_START, KOTH_END)],
    RK: [RK_CATCH, (RK_HOME, ""), (RK_START, RK_ENDS[0]), (RK_START, RK_ENDS[1])],
}


def games_of(v):
    """About six random legal games of 20-60 plies, then the hand-made ones."""
    return [(START[v], F.random_vgame(300 + 10 * v + i, v, START[v], 20 + 8 * i)) for i in range(6)] + HAND[v]


GAMES = {v: games_of(v) for v in VARIANTS}


def wrap_neg(x):
    return ((-int(x) + 2**31) % 2**32) - 2**31


def trunc_div(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)


def child_key(ps, po, end, x, c, low_bits_only=False):
    """(rank, value) of a child by the rule of fnnue.h; with low_bits_only the rule as it was before ABI 3.6."""
    f = int(end[x])
    if low_bits_only:
        if f & F.END_NO_MOVES:
            return (2, 0) if f & F.END_CHECK else (1, 0)
        return (1, -trunc_div(int(ps[x]) + int(po[x]), 16))
    if f & WON:
        return (0, 0)
    if f & F.END_NO_MOVES:
        return (2, 0) if f & DECIDED else (1, 0)
    return (1, -trunc_div(int(ps[x]) + int(po[x]), 16))


KIND = {0: F.BEST_LOST, 1: F.BEST_CP, 2: F.BEST_MATE}


def reduce_groups(ps, po, end, moves, off, low_bits_only=False):
    """fnnue_best_children in Python: BEST_DTYPE tuples."""
    out, npos = [], len(ps)
    for g in range(len(off) - 1):
        e = min(int(off[g + 1]), npos)
        o = min(int(off[g]), e)
        if o == e:
            out.append((0,) * 8)
            continue
        best, key = 0, None
        for c in range(1, e - o):
            k = child_key(ps, po, end, o + c, c, low_bits_only)
            if key is None or k > key:  # the first maximum
                best, key = c, k
        if not best:
            out.append((0, 0, 0, e - o - 1, 0, 0, F.BEST_NONE, int(end[o])))
            continue
        kind = KIND[key[0]]
        out.append((wrap_neg(ps[o + best]), wrap_neg(po[o + best]), key[1] if kind == F.BEST_CP else 0, e - o - 1, best,
                    int(moves[o + best]) if moves is not None else 0, kind, int(end[o])))
    return out


def ranked(ps, po, end, moves, o, e, low_bits_only=False):
    """The children of [o, e) in fnnue_topk_children's order, as LINE_DTYPE tuples."""
    keys = [child_key(ps, po, end, o + c, c, low_bits_only) + (-c,) for c in range(1, e - o)]
    out = []
    for rank, value, c in sorted(keys, reverse=True):
        c = -c
        out.append((wrap_neg(ps[o + c]), wrap_neg(po[o + c]), value if rank == 1 else 0, c,
                    int(moves[o + c]) if moves is not None else 0, KIND[rank], 0))
    return out


def topk_groups(ps, po, end, moves, off, k, low_bits_only=False):
    """fnnue_topk_children with k slots per group in Python: (ngroups, k) LINE_DTYPE tuples, zero where unused."""
    out, npos = [], len(ps)
    for g in range(len(off) - 1):
        e = min(int(off[g + 1]), npos)
        o = min(int(off[g]), e)
        order = ranked(ps, po, end, moves, o, e, low_bits_only) if e > o else []
        out.append((order + [(0,) * 7] * k)[:k])
    return out


def as_tuples(recs):
    return [tuple(int(r[n]) for n in recs.dtype.names) for r in recs]


def line_tuples(lines):
    return [as_tuples(row) for row in lines]


@pytest.fixture(scope="module")
def data():
    return {ZH: F.synthesize_variant_net(5, 256, ZH), AT: F.synthesize_variant_net(6, 256, AT),
            KOTH: F.synthesize_variant_net(7, 256, KOTH), RK: F.synthesize_variant_net(8, 256, RK)}


@pytest.fixture(scope="module")
def evs(data):
    """A crazyhouse and an atomic context (the atomic net also serves kingOfTheHill and racingKings), and
    contexts of the two plain variants' own nets (the actor's)."""
    made = {v: F.Evaluator(F.Net.from_bytes_variant(data[v], v), 0) for v in VARIANTS}
    yield made
    for e in made.values():
        e.close()


def serving(evs, v):
    return evs[ZH] if v == ZH else evs[AT]


@pytest.fixture(scope="module")
def kids(evs):
    """Per variant: the device's children of GAMES[v] (computed once, never changed)."""
    out = {}
    for v in VARIANTS:
        pos, off, moves, end = serving(evs, v).build_vchildren(v, GAMES[v])
        for a in (pos, off, moves, end):
            a.setflags(write=False)
        first, g0 = [], 0
        for _, m in GAMES[v]:
            first.append(g0)
            g0 += len(m.split()) + 1
        assert g0 == len(off) - 1
        out[v] = (pos, off, moves, end, first)
    return out


# ---- the builder against the host ----

def test_games_are_what_they_should_be():
    for v in VARIANTS:
        lens = [len(m.split()) for _, m in GAMES[v][:6]]
        assert max(lens) >= 40 and min(lens) >= 10, (v, lens)
    assert F.game_end(*ZH_MATE, ZH) == F.END_NO_MOVES | F.END_CHECK
    assert F.game_end(*ZH_BLOCK, ZH) == F.END_CHECK
    assert F.game_end(CHESS_START, ATOMIC_WIN, AT) & F.END_EXTINCT
    assert F.game_end(CHESS_START, KOTH_END, KOTH) == F.END_NO_MOVES | F.END_VARIANT


@pytest.mark.parametrize("v", VARIANTS)
def test_records_and_offsets_equal_host_and_plain_builder(evs, kids, v):
    pos, off, moves, end, first = kids[v]
    p2, o2 = serving(evs, v).build_vbatch(v, GAMES[v], F.PLAYOUT_CHILDREN)
    assert np.array_equal(pos, p2) and np.array_equal(off, o2)
    for (fen, mv), g0 in zip(GAMES[v], first):
        hp, ho = F.game_vchildren(v, fen, mv)
        n = len(ho) - 1
        assert np.array_equal(off[g0:g0 + n + 1] - off[g0], ho)
        assert np.array_equal(pos[off[g0]:off[g0 + n]], hp)


def nib(p, s):
    return (int(p[s >> 1]) >> (4 * (s & 1))) & 15


def king_rank(p, colour):
    for s in range(64):
        if nib(p, s) == (colour << 3 | 6):
            return s >> 3
    return -1


@pytest.mark.parametrize("v", VARIANTS)
def test_moves_and_end_flags_against_host_replays(kids, v):
    """Each child's move text, replayed after the game's prefix, is legal and gives exactly that record; each
    record's flags are the host's for the same prefix; END_WON exactly on the racingKings children in which
    white, to move, stands on rank 8 and black does not."""
    pos, off, moves, end, first = kids[v]
    replays, won, drops, texts_seen = 0, 0, 0, set()
    for (fen, mv), g0 in zip(GAMES[v], first):
        ms = mv.split()
        for q in range(len(ms) + 1):
            o, e = int(off[g0 + q]), int(off[g0 + q + 1])
            prefix = ms[:q]
            assert moves[o] == 0
            assert end[o] == F.game_end(fen, prefix, v), (fen, prefix)
            assert not end[o] & WON
            assert bool(end[o] & F.END_NO_MOVES) == (e - o == 1)
            texts = [F.vmove_uci(int(m)) for m in moves[o + 1:e]]
            assert len(set(texts)) == len(texts) and "" not in texts
            for x, t in zip(range(o + 1, e), texts):
                assert int(end[x]) & ~WON == F.game_end(fen, prefix + [t], v), (fen, prefix, t)
                assert np.array_equal(F.game_vpositions(v, fen, prefix + [t])[-1], pos[x]), (fen, prefix, t)
                is_won = v == RK and int(pos[x][32]) == 0 and king_rank(pos[x], 0) == 7 and king_rank(pos[x], 1) != 7
                assert bool(end[x] & WON) == is_won, (fen, prefix, t)
                won += is_won
                drops += "@" in t
                replays += 1
            texts_seen.update(texts)
            if q < len(ms):
                assert ms[q] in texts  # the game's own notation
    assert replays > 1500
    assert (won > 0) == (v == RK)
    assert (drops > 0) == (v == ZH)
    if v == ZH:
        g = first[6]  # full pockets: every piece type drops, pawns on ranks 2-7 only
        t0 = [F.vmove_uci(int(m)) for m in moves[off[g] + 1:off[g + 1]]]
        assert {t[0] for t in t0 if "@" in t} == set("PNBRQ")
        assert all(t[3] not in "18" for t in t0 if t.startswith("P@")) and "N@b8" in t0 and "Q@b1" in t0 and "N@a8" not in t0
        assert len(t0) > 256  # beyond the top-k kernel's register path
        o = int(off[first[7] + 1])  # after R@e8: mate; with a black rook in hand two drops block
        assert end[o] == F.END_NO_MOVES | F.END_CHECK
        o, e = int(off[first[8] + 1]), int(off[first[8] + 2])
        assert sorted(F.vmove_uci(int(m)) for m in moves[o + 1:e]) == ["R@f8", "R@g8"] and end[o] == F.END_CHECK
    if v == AT:
        g = first[6] + 4  # before Nxf7
        o, e = int(off[g]), int(off[g + 1])
        boom = [x for x in range(o + 1, e) if F.vmove_uci(int(moves[x])) == "g5f7"]
        assert len(boom) == 1 and end[boom[0]] & F.END_EXTINCT and end[boom[0]] & F.END_NO_MOVES
        t0 = [F.vmove_uci(int(m)) for m in moves[off[first[9]] + 1:off[first[9] + 1]]]
        assert "f1a1" in t0 and "f1g1" in t0  # Chess960 castling: the king takes its rook
    if v == KOTH:
        o, e = int(off[first[6]]), int(off[first[6] + 1])
        hill = {F.vmove_uci(int(moves[x])) for x in range(o + 1, e) if end[x] == F.END_NO_MOVES | F.END_VARIANT}
        assert hill == {"d3d4", "d3e4"}
    if v == RK:
        o, e = int(off[first[6] + 1]), int(off[first[6] + 2])  # after a7a8: black to move
        flags = {F.vmove_uci(int(moves[x])): int(end[x]) for x in range(o + 1, e)}
        assert len(flags) == 5 and sorted(t for t, f in flags.items() if f & WON) == ["h7g6", "h7g7", "h7h6"]
        assert flags["h7g8"] == F.END_NO_MOVES and flags["h7h8"] == F.END_NO_MOVES  # both home: a draw


# ---- the reduction ----

def hand_made_groups():
    ps, po, end, off = [], [], [], [0]

    def group(p, q, f):
        ps.extend(p), po.extend(q), end.extend(f)
        off.append(len(ps))

    group([0, 160, 160], [0, 0, 0], [0, 5, 0])                     # 0: an exploded king (1 | 4): mate
    group([0, -16000, 0], [0, 0, 0], [0, 0, 9])                    # 1: a variant win behind a large value
    group([0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 13, 9])               # 2: stalemate, then two mates: the first mate
    group([0, 7, 7, 7], [0, 0, 0, 0], [0, WON, WON, 0x41])         # 3: all WON: the first, kind 3
    group([0, 50, 0, 320], [0, 0, 0, 0], [0, WON, 1, 0])           # 4: WON beside a stalemate and a negative value
    group([0, 320, 640], [0, 0, 0], [0, 0x41, 0])                  # 5: WON | NO_MOVES beside negative values only
    group([0, 0, 0], [0, 0, 0], [0, 0x49, 9])                      # 6: WON | NO_MOVES | VARIANT loses to a mate
    group([0, 0, 0], [0, 0, 0], [0, 0x4B, 0x43])                   # 7: WON with every other bit: still lost
    group([0, -999, 16], [0, 0, 0], [0, 4, 8])                     # 8: bits 2 / 3 without NO_MOVES: evaluated
    group([3, 1, 2], [0, 0, 0], [9, 2, 0])                         # 9: a check alone is evaluated; parent's end 9
    group([5], [5], [5])                                           # 10: no child
    group([], [], [])                                              # 11: empty
    group([0] + [16 * i for i in range(40)], [0] * 41, [0] + [WON if i % 3 else 0 for i in range(40)])  # 12
    n = len(ps)
    return (np.array(ps, dtype=np.int32), np.array(po, dtype=np.int32), np.array(end, dtype=np.uint8),
            (np.arange(n) * 73 % 4096 + 64).astype(np.uint16), np.array(off, dtype=np.uint32))


def test_reduction_variant_ranks_on_hand_made_groups(evs):
    ev = evs[AT]
    ps, po, end, moves, off = hand_made_groups()
    got = as_tuples(ev.best_children(ps, po, end, moves, off))
    assert got == reduce_groups(ps, po, end, moves, off)
    rec = lambda g: dict(zip(F.BEST_DTYPE.names, got[g]))
    assert (rec(0)["kind"], rec(0)["best"], rec(0)["value"]) == (F.BEST_MATE, 1, 0)
    assert (rec(1)["kind"], rec(1)["best"]) == (F.BEST_MATE, 2)
    assert (rec(2)["kind"], rec(2)["best"]) == (F.BEST_MATE, 2)
    assert (rec(3)["kind"], rec(3)["best"], rec(3)["value"], rec(3)["psqt"]) == (F.BEST_LOST, 1, 0, -7)
    assert (rec(4)["kind"], rec(4)["best"], rec(4)["value"]) == (F.BEST_CP, 2, 0)
    assert (rec(5)["kind"], rec(5)["best"], rec(5)["value"]) == (F.BEST_CP, 2, -40)
    assert (rec(6)["kind"], rec(6)["best"]) == (F.BEST_MATE, 2)
    assert (rec(7)["kind"], rec(7)["best"]) == (F.BEST_LOST, 1)
    assert (rec(8)["kind"], rec(8)["best"], rec(8)["value"]) == (F.BEST_CP, 1, 62)
    assert (rec(9)["kind"], rec(9)["best"], rec(9)["end"]) == (F.BEST_CP, 1, 9)
    assert rec(10)["kind"] == F.BEST_NONE and rec(10)["end"] == 5 and got[11] == (0,) * 8
    assert (rec(12)["kind"], rec(12)["best"], rec(12)["value"]) == (F.BEST_CP, 1, 0)
    assert as_tuples(ev.best_children(ps, po, end, None, off)) == reduce_groups(ps, po, end, None, off)
    for k in (1, 3, 40):
        lines, _ = ev.topk_children(ps, po, end, moves, off, k)
        assert line_tuples(lines.reshape(len(off) - 1, k)) == topk_groups(ps, po, end, moves, off, k)
    lines, _ = ev.topk_children(ps, po, end, moves, off, 3)
    lines = lines.reshape(len(off) - 1, 3)
    assert [int(x) for x in lines[3]["kind"]] == [F.BEST_LOST] * 3 and [int(x) for x in lines[3]["child"]] == [1, 2, 3]
    assert [int(x) for x in lines[4]["kind"]] == [F.BEST_CP, F.BEST_CP, F.BEST_LOST]
    assert [int(x) for x in lines[4]["child"]] == [2, 3, 1] and int(lines[4]["value"][2]) == 0


def test_reduction_is_unchanged_for_chess_flag_bytes(evs):
    """End bytes that use bits 0 and 1 only: both kernels give what the rule restricted to those bits gives
    (the arrays of the chess tests: random values, ties, mates, stalemates, 64-bit sums, sizes up to 219)."""
    ev = evs[ZH]
    rng = np.random.default_rng(5)
    ps, po, end, off = [], [], [], [0]

    def group(p, q, f):
        ps.extend(p), po.extend(q), end.extend(f)
        off.append(len(ps))

    for size in (0, 1, 2, 33, 64, 65, 219):
        group(rng.integers(-40000, 40000, size), rng.integers(-40000, 40000, size), rng.integers(0, 4, size))
    group([0] + [160] * 40, [0] + [-320] * 40, [0] * 41)
    group([5, -16 * 10**6, 7, 9], [0, 0, 0, 0], [0, 0, 0, 3])
    group([0, 100, 900, 16, 40], [0, 60, 0, 16, 0], [0, 0, 0, 1, 0])
    group([0, 17, 1, -17, 1], [0, 0, 0, 0, 0], [0] * 5)
    group([0, 2**31 - 1, 0], [0, 2**31 - 1, 0], [2, 0, 0])
    group([0, 0, -2**31], [0, 0, -2**31], [0, 0, 0])
    group([0, 2**31 - 1, 2**31 - 1], [0, -2**31, -2**31 + 16], [0, 0, 0])
    group([0, 0, 0, 0], [0, 0, 0, 0], [0, 3, 3, 1])
    group([0, 0, 0], [0, 0, 0], [3, 2, 2])
    ps = np.array(ps, dtype=np.int64).astype(np.int32)
    po = np.array(po, dtype=np.int64).astype(np.int32)
    end = np.array(end, dtype=np.uint8)
    off = np.array(off, dtype=np.uint32)
    moves = (np.arange(len(ps)) * 73 % 4096 + 64).astype(np.uint16)
    assert int(end.max()) <= 3
    want = reduce_groups(ps, po, end, moves, off, low_bits_only=True)
    assert want == reduce_groups(ps, po, end, moves, off)
    assert as_tuples(ev.best_children(ps, po, end, moves, off)) == want
    for k in (1, 5, 218):
        lines, _ = ev.topk_children(ps, po, end, moves, off, k)
        assert line_tuples(lines.reshape(len(off) - 1, k)) == topk_groups(ps, po, end, moves, off, k, True)


@pytest.mark.parametrize("nrec", [0, 1, 2, 33, 257, 258, 600])
def test_topk_sizes_with_the_new_flags(evs, nrec):
    """One group of nrec records between two small ones; 257 records = 256 children is the last size of the
    register path, 258 the first of the other."""
    ev = evs[AT]
    rng = np.random.default_rng(nrec)
    sizes = [3, nrec, 4]
    n = sum(sizes)
    ps = rng.integers(-3000, 3000, n).astype(np.int32)
    po = rng.integers(-3000, 3000, n).astype(np.int32)
    end = rng.choice(np.array([0, 0, 0, 0, 1, 2, 5, 9, 13, WON, 0x41, 0x49], dtype=np.uint8), n)
    moves = (np.arange(n) * 37 % 4000 + 65).astype(np.uint16)
    off = np.cumsum([0] + sizes).astype(np.uint32)
    assert as_tuples(ev.best_children(ps, po, end, moves, off)) == reduce_groups(ps, po, end, moves, off)
    for k in (1, 7, 218):
        lines, _ = ev.topk_children(ps, po, end, moves, off, k)
        lines = lines.reshape(3, k)
        want = topk_groups(ps, po, end, moves, off, k)
        assert line_tuples(lines) == want
        best = as_tuples(ev.best_children(ps, po, end, moves, off))
        for g in range(3):  # slot 0 is the group's fnnue_best
            if best[g][6] != F.BEST_NONE:
                l = want[g][0]
                assert (l[0], l[1], l[2], l[3], l[4], l[5]) == (best[g][0], best[g][1], best[g][2], best[g][4],
                                                                best[g][5], best[g][6])


# ---- vsearch1 / vsearch1_lines ----

@pytest.fixture(scope="module")
def searched(evs, kids):
    """Per variant: vsearch1_lines(k = 3) of GAMES[v], and its three steps done one by one."""
    out = {}
    for v in VARIANTS:
        ev = serving(evs, v)
        pos, off, moves, end, first = kids[v]
        ps, po = ev.eval_vgroups(pos, off, N.GROUP_STAR)
        want = as_tuples(ev.best_children(ps, po, end, moves, off))
        lines, _ = ev.topk_children(ps, po, end, moves, off, 3)
        best, goff, got_lines = ev.vsearch1_lines(v, GAMES[v], 3)
        for a in (best, goff, got_lines):
            a.setflags(write=False)
        out[v] = (best, goff, got_lines, want, line_tuples(lines.reshape(len(off) - 1, 3)), (ps, po))
    return out


@pytest.mark.parametrize("v", VARIANTS)
def test_vsearch1_equals_its_three_steps(evs, kids, searched, v):
    best, goff, lines, want, want_lines, (ps, po) = searched[v]
    pos, off, moves, end, first = kids[v]
    assert goff.tolist() == first + [len(off) - 1]
    assert as_tuples(best) == want
    assert line_tuples(lines) == want_lines
    # the device's own steps against the restatement of the rule
    assert want == reduce_groups(ps, po, end, moves, off)
    assert want_lines == topk_groups(ps, po, end, moves, off, 3)
    b2, g2 = serving(evs, v).vsearch1(v, GAMES[v])
    assert np.array_equal(b2, best) and np.array_equal(g2, goff)
    kinds = {int(r["kind"]) for r in best}
    assert F.BEST_CP in kinds and F.BEST_MATE in kinds and F.BEST_NONE in kinds


def test_vsearch1_special_plies(searched, kids):
    best, goff = searched[RK][0], searched[RK][1]
    r = best[goff[6] + 1]  # black must catch up: a draw; the three losing moves are never chosen
    assert (r["kind"], r["value"], r["nodes"]) == (F.BEST_CP, 0, 5) and F.vmove_uci(int(r["move"])) in ("h7g8", "h7h8")
    lines = searched[RK][2][goff[6] + 1]
    assert [int(k) for k in lines["kind"]] == [F.BEST_CP, F.BEST_CP, F.BEST_LOST]
    r = best[goff[9] - 1]   # white home, black cannot catch up: over, lost
    assert (r["kind"], r["end"]) == (F.BEST_NONE, F.END_NO_MOVES | F.END_VARIANT)
    r = best[goff[10] - 1]  # both home: a draw
    assert (r["kind"], r["end"]) == (F.BEST_NONE, F.END_NO_MOVES)
    best, goff = searched[AT][0], searched[AT][1]
    r = best[goff[6] + 4]
    assert (r["kind"], F.vmove_uci(int(r["move"]))) == (F.BEST_MATE, "g5f7")
    r = best[goff[6] + 5]
    assert r["kind"] == F.BEST_NONE and r["end"] & F.END_EXTINCT
    best, goff = searched[KOTH][0], searched[KOTH][1]
    assert (best[goff[6]]["kind"], F.vmove_uci(int(best[goff[6]]["move"]))) == (F.BEST_MATE, "d3d4")
    best, goff = searched[ZH][0], searched[ZH][1]
    assert best[goff[6]]["nodes"] > 256
    mate = F.vmove_uci(int(best[goff[7]]["move"]))  # the first mating drop in generation order (a8 ... f8)
    assert best[goff[7]]["kind"] == F.BEST_MATE and mate[:2] == "R@" and mate[3] == "8"
    assert F.game_end(ZH_MATE[0], mate, ZH) == F.END_NO_MOVES | F.END_CHECK
    assert best[goff[8] + 1]["nodes"] == 2 and searched[ZH][2][goff[8] + 1]["kind"][2] == F.BEST_NONE


def test_vsearch1_arch_and_capacity(evs, searched):
    games = GAMES[KOTH][:2]
    chess = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
    try:
        for v in VARIANTS:
            with pytest.raises(F.FnnueError) as err:
                chess.vsearch1(v, games)
            assert err.value.code == -4
        with pytest.raises(F.FnnueError) as err:  # fnnue_search1 stays a chess entry point
            evs[AT].search1(games)
        assert err.value.code == -4
    finally:
        chess.close()
    for ev, v in ((evs[AT], ZH), (evs[ZH], AT), (evs[ZH], KOTH), (evs[KOTH], AT), (evs[KOTH], RK), (evs[AT], 0),
                  (evs[AT], 9)):
        with pytest.raises(F.FnnueError) as err:
            ev.vsearch1(v, games)
        assert err.value.code == -4, v
    b, g = evs[KOTH].vsearch1(KOTH, games)  # a net of the variant's own id
    b2, _ = evs[AT].vsearch1(KOTH, games)
    assert len(b) == len(b2) == sum(len(m.split()) + 1 for _, m in games)
    # one record short: FNNUE_E_CAPACITY, sizes reported, nothing written
    text, fen_off, mv_off = F.pack_games(games)
    plies = len(b)
    out = np.full(plies * N.BEST_BYTES, 0xA5, dtype=np.uint8)
    off = np.full(len(games) + 1, 0xA5A5A5A5, dtype=np.uint32)
    import ctypes as C
    n, gg = C.c_size_t(), C.c_size_t()
    rc = N.lib.fnnue_vsearch1(evs[AT]._h, KOTH, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), N.ptr(out),
                              plies - 1, N.ptr(off), len(off), C.byref(n), C.byref(gg))
    assert rc == -10 and n.value == plies and gg.value == len(games)
    assert (out == 0xA5).all() and (off == 0xA5A5A5A5).all()
    lines = np.full(plies * 2 * N.LINE_BYTES, 0xA5, dtype=np.uint8)
    rc = N.lib.fnnue_vsearch1_lines(evs[AT]._h, KOTH, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), 2,
                                    N.ptr(out), plies, N.ptr(off), len(off), N.ptr(lines), plies * 2 - 1, C.byref(n),
                                    C.byref(gg))
    assert rc == -10 and n.value == plies and (out == 0xA5).all() and (lines == 0xA5).all()
    with pytest.raises(F.FnnueError) as err:
        evs[AT].vsearch1(AT, [(CHESS_START, "e2e4"), (CHESS_START, "e2e4 e2e4")])
    assert err.value.code == -8 and "game 1" in str(err.value)


def test_vsearch1_device_form_is_identical(evs, searched):
    import torch
    best, goff, lines = searched[ZH][:3]
    ev = evs[ZH]
    dev = torch.device("cuda", 0)
    text, fen_off, mv_off = F.pack_games(GAMES[ZH])
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    ng = len(GAMES[ZH])
    d_off = torch.zeros(ng + 1, dtype=torch.int32, device=dev)
    d_out = torch.zeros(len(best) * N.BEST_BYTES, dtype=torch.uint8, device=dev)
    d_lines = torch.zeros(len(best) * 3 * N.LINE_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(F.FnnueError) as err:
        ev.vsearch1_device(ZH, d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, 0, 0, d_off.data_ptr(), ng + 1,
                           None)
    assert err.value.code == -10
    n, g = ev.vsearch1_lines_device(ZH, d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, 3, d_out.data_ptr(),
                                    len(best), d_off.data_ptr(), ng + 1, d_lines.data_ptr(), len(best) * 3, None)
    ev.check()
    assert (n, g) == (len(best), ng)
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST_DTYPE), best)
    assert np.array_equal(d_lines.cpu().numpy().view(F.LINE_DTYPE).reshape(-1, 3), lines)
    assert d_off.cpu().numpy().tolist() == goff.tolist()
    # the children builder's device form: a sizing call, then the same arrays as the host form
    rc, nrec, ngr = ev.build_vchildren_device(ZH, d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, 0, 0, 0, 0,
                                              0, 0, None)
    assert rc == -10 and ngr == len(best)
    d_pos = torch.zeros(nrec * N.VPOS_BYTES, dtype=torch.uint8, device=dev)
    d_goff = torch.zeros(ngr + 1, dtype=torch.int32, device=dev)
    d_mv = torch.zeros(nrec, dtype=torch.int16, device=dev)
    d_end = torch.zeros(nrec, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rc, n2, g2 = ev.build_vchildren_device(ZH, d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng,
                                           d_pos.data_ptr(), nrec, d_goff.data_ptr(), ngr + 1, d_mv.data_ptr(),
                                           d_end.data_ptr(), None)
    assert (rc, n2, g2) == (0, nrec, ngr)
    pos, off, moves, end = ev.build_vchildren(ZH, GAMES[ZH])
    assert np.array_equal(d_pos.cpu().numpy().reshape(-1, N.VPOS_BYTES), pos)
    assert np.array_equal(d_goff.cpu().numpy().view(np.uint32), off)
    assert np.array_equal(d_mv.cpu().numpy().view(np.uint16), moves) and np.array_equal(d_end.cpu().numpy(), end)


# ---- the engine actor ----

def make_channel(data, **kw):
    return B.channel(F.Net.from_bytes(net_bytes(1, 256, 0)), 0, crazyhouse=F.Net.from_bytes_variant(data[ZH], ZH),
                     atomic=F.Net.from_bytes_variant(data[AT], AT),
                     kingofthehill=F.Net.from_bytes_variant(data[KOTH], KOTH),
                     racingkings=F.Net.from_bytes_variant(data[RK], RK), **kw)


@pytest.fixture(scope="module")
def chans(data):
    """(a channel at variant analysis depth 1, a channel never set), chess and the four variant nets."""
    made = [make_channel(data, variant_analysis_depth=1), make_channel(data)]
    yield made[0][0], made[1][0]
    for _, actor in made:
        actor.close()


def body(v, tag, fen, moves, **kw):
    return B.AcquireResponseBody(tag, fen, moves, variant=NAME[v], **kw)


def analysis_bodies():
    bodies, kinds = [], []
    for v in VARIANTS:
        for i, (fen, mv) in enumerate(GAMES[v]):
            bodies.append(body(v, f"{NAME[v]}{i}", fen, mv))
            kinds.append(v)
    return bodies, kinds


CHESS_BODIES = [B.AcquireResponseBody("c0", CHESS_START, "e2e4 e7e5 g1f3 b8c6"),
                B.AcquireResponseBody("c1", CHESS_START, "f2f3 e7e5 g2g4 d8h4"),
                B.AcquireResponseBody("cm", CHESS_START, "e2e4 e7e5", work="move")]


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


@pytest.fixture(scope="module")
def answers(chans):
    d1, d0 = chans
    bodies, kinds = analysis_bodies()
    res, zero = d1.go(bodies), d0.go(bodies)
    return bodies, kinds, res, zero


def test_actor_depth1_equals_move_work_of_every_prefix(chans, answers):
    """The oracle is the project's own move work: the depth-1 response of ply q equals the response of a
    work = "move" batch over the first q moves.  A ply without a legal move is answered as at depth 0 (the
    header's rule): its score, depth 0, nodes 0 and missing move are move work's, and its psqt / positional are
    the ply's own terms as the depth-0 channel reports them (move work reports none for such a root)."""
    d1, d0 = chans
    bodies, kinds, res, zero = answers
    roots, where = [], []
    for i, (b, v) in enumerate(zip(bodies, kinds)):
        ms = b.moves.split()
        for q in range(len(ms) + 1):
            roots.append(body(v, f"{b.batch_id}.{q}", b.position, " ".join(ms[:q]), work="move"))
            where.append((i, q))
    moved = d0.go(roots)
    seen = {"terminal": 0, "mate": 0, "drop": 0}
    for (i, q), m in zip(where, moved):
        assert not isinstance(res[i], B.PositionFailed) and not isinstance(m, B.PositionFailed), bodies[i].batch_id
        r, z, m = res[i][q], zero[i][q], m[0]
        assert r.position_id == q
        assert (r.score, r.depth, r.nodes, r.best_move) == (m.score, m.depth, m.nodes, m.best_move), (bodies[i], q)
        if m.depth == 0:
            assert (m.nodes, m.best_move, z.depth, z.nodes) == (0, None, 0, 0)
            assert (r.psqt, r.positional) == (z.psqt, z.positional) and r.score == z.score
            seen["terminal"] += 1
        else:
            assert (r.psqt, r.positional) == (m.psqt, m.positional), (bodies[i], q)
            assert r.depth == 1 and z.depth == 0 and z.nodes == 1
        seen["mate"] += r.score == B.Score("mate", 1)
        seen["drop"] += "@" in (r.best_move or "")
    assert all(seen.values()), seen
    assert strip(d1.go(bodies)) == strip(res)  # the same go() twice


def test_actor_back_to_zero_and_chess_unaffected(chans, answers):
    d1, d0 = chans
    bodies, kinds, res, zero = answers
    mixed = bodies[::3] + CHESS_BODIES
    try:
        d1.set_variant_analysis_depth(0)
        assert strip(d1.go(mixed)) == strip(d0.go(mixed))
        # chess depth is its own setting: variant batches stay at depth 0 under it (and the reverse)
        d1.set_analysis_depth(1)
        d0.set_analysis_depth(1)
        both0 = d1.go(mixed)
        assert strip(both0) == strip(d0.go(mixed)) and both0[-3][0].depth == 1 and both0[0][0].depth == 0
        d1.set_variant_analysis_depth(1)
        both1 = d1.go(mixed)
        assert strip(both1[-3:]) == strip(both0[-3:]) and both1[0][0].depth == 1
        d1.set_analysis_depth(0)
        d0.set_analysis_depth(0)
        chess0 = d1.go(mixed)
        assert strip(chess0[-3:]) == strip(d0.go(CHESS_BODIES)) and chess0[-3][0].depth == 0
        assert strip(chess0[:-3]) == strip(both1[:-3]) == strip(res[::3])
    finally:
        d1.set_analysis_depth(0)
        d0.set_analysis_depth(0)
        d1.set_variant_analysis_depth(1)
    with pytest.raises(F.FnnueError) as err:
        d1.set_variant_analysis_depth(2)
    assert err.value.code == -1
    # move work is the same at either depth
    mv = [body(RK, "mv", *RK_CATCH, work="move"), body(ZH, "mvz", ZH_POCKETS, "", work="move")]
    assert strip(d1.go(mv)) == strip(d0.go(mv))


def test_actor_illegal_move_fails_alone(chans, answers):
    d1, _ = chans
    bodies, kinds, res, _ = answers
    pick = [0, 10, 20, 30]
    mixed = [bodies[pick[0]], body(ZH, "bad", ZH_START, "e2e4 e7e5 P@e3"), bodies[pick[1]],
             body(AT, "bad2", CHESS_START, "e2e4 e7e5 e1e3"), bodies[pick[2]], bodies[pick[3]],
             body(RK, "check", RK_START, "e2c3"), CHESS_BODIES[0]]
    got = d1.go(mixed)
    assert [getattr(r, "code", 0) for r in got] == [0, -8, 0, -8, 0, 0, -8, 0]
    assert strip([got[0], got[2], got[4], got[5]]) == strip([res[i] for i in pick])
    assert B.last_stats(d1._actor)["rebuilds"] >= 1


def test_actor_skipped_and_compact(chans, answers):
    d1, _ = chans
    bodies, kinds, res, _ = answers
    b = bodies[0]
    rows = d1.go([body(ZH, "s", b.position, b.moves, skip_positions=[1, 3])])[0]
    assert [r.skipped for r in rows[:4]] == [False, True, False, True]
    assert strip([rows[4:]]) == strip([res[0][4:]]) and rows[0].best_move == res[0][0].best_move
    some = bodies[::4]
    for rows, crows in zip(d1.go(some), d1.go_compact(some)):
        assert [(r.score, r.depth, r.psqt, r.positional) for r in rows] == \
            [(r.score, r.depth, r.psqt, r.positional) for r in crows]
        assert all(r.best_move is None for r in crows)


def test_actor_go_lines(chans, evs, searched):
    d1, d0 = chans
    for v in VARIANTS:
        games = GAMES[v][3:]
        bodies = [body(v, f"l{i}", fen, mv, multipv=3) for i, (fen, mv) in enumerate(games)]
        assert B.lines_bound(bodies) == 3 * sum(len(m.split()) + 1 for _, m in games)
        res = d1.go_lines(bodies)
        plain = d1.go(bodies)
        best, goff, lines = evs[v].vsearch1_lines(v, games, 3)  # the actor's own net of the variant
        for i, rows in enumerate(res):
            assert not isinstance(rows, B.PositionFailed)
            for q, r in enumerate(rows):
                b, ls = best[goff[i] + q], lines[goff[i] + q]
                if b["kind"] == F.BEST_NONE:
                    assert r.lines is None and r.depth == 0
                    continue
                assert len(r.lines) == min(3, int(b["nodes"]))
                assert (r.lines[0].score, r.lines[0].move, r.lines[0].psqt, r.lines[0].positional) == \
                    (r.score, r.best_move, r.psqt, r.positional)
                for l, d in zip(r.lines, ls):
                    score = {F.BEST_MATE: B.Score("mate", 1), F.BEST_LOST: B.Score("mate", -1)}.get(
                        int(d["kind"]), B.Score("cp", trunc_div(int(d["value"]) * 100, NORM)))
                    assert (l.score, l.move, l.psqt, l.positional) == \
                        (score, F.vmove_uci(int(d["move"])), int(d["psqt"]), int(d["positional"]))
            assert strip([rows]) == strip([plain[i]])
        assert all(r.lines is None for rows in d0.go_lines(bodies) for r in rows)
    rows = d1.go_lines([body(ZH, "two", *ZH_BLOCK, multipv=3)])[0]
    assert rows[1].nodes == 2 and sorted(l.move for l in rows[1].lines) == ["R@f8", "R@g8"]
    parts = json.loads(B.into_analysis(d1.go([body(ZH, "pv", *ZH_BLOCK)])[0]))
    assert parts[1]["pv"] in ("R@f8", "R@g8") and parts[1]["depth"] == 1 and "@" in parts[0]["pv"] + parts[1]["pv"]


def test_actor_small_pieces_give_the_same_answers(monkeypatch, data, answers):
    """FNNUE_BACKEND_PIECE_PLIES = 1024 cuts variant depth-1 pieces at 256 plies: a call with a few hundred
    plies per net spans several pieces per net, a failing game in a middle piece is restaged, and every
    answer is what the one-piece call gave."""
    bodies, kinds, res, _ = answers
    monkeypatch.setenv("FNNUE_BACKEND_PIECE_PLIES", "1024")
    stub, actor = make_channel(data, variant_analysis_depth=1)
    try:
        twice = bodies + [body(AT, "bad", CHESS_START, "e2e4 e7e5 e1e3")] + bodies
        got = stub.go(twice)
        st = B.last_stats(actor)
        assert st["pieces"] >= 8 and st["rebuilds"] >= 1, st  # four nets, about 500 plies each, cut at 256
        n = len(bodies)
        assert isinstance(got[n], B.PositionFailed) and got[n].code == -8
        assert strip(got[:n]) == strip(res) and strip(got[n + 1:]) == strip(res)
    finally:
        actor.close()

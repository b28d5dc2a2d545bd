"""Repetition and fifty-move draws, the host side (ABI 3.12): the layout of
fnnue_ply_history, the no-device error paths of the new entry points,
F.game_history against a tracker written here, and the rule of include/fnnue.h
restated in Python: tests/test_search2.py's reduce_group and reply_rule extended
with FNNUE_END_DRAW, and a host-built reference of the searches with the draw
rules on (what tests/test_gpu_draws.py holds the device to)."""
import ctypes as C

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet
from tests import test_multipv2 as M2
from tests import test_search2 as R
from tests.conftest import net_bytes
from tests.positions import CHESS960, START

E_ARG = -1
BEST = R.BEST
SHUFFLE = "g1f3 g8f6 f3g1 f6g8"
ROOKS = "h2h4 h7h5 h1h2 h8h7 h2h1 h7h8 h1h2 h8h7 h2h1 h7h8"
KNIGHTS_BACK = "d7d5 g1f3 g8f6 f3g1 f6g8"
E5 = "rnbqkbnr/pppppppp/8/4P3/8/8/PPPP1PPP/RNBQKBNR b KQkq - 0 3"   # d7d5: the e5 pawn attacks d6
A5 = "rnbqkbnr/pppppppp/8/P7/8/8/1PPPPPPP/RNBQKBNR b KQkq - 0 3"    # d7d5: nobody attacks d6
LONE_EP = "rnbqkbnr/pppp1ppp/8/4p3/8/8/PPPPPPPP/RNBQKBNR w KQkq e6 0 2"  # e6 named, no white pawn beside e5
KRK = "7k/5K2/6R1/8/8/8/8/8 w - - {} 80"                             # Rh6 mates; Rg7 stalemates
PAWNS = "7k/8/8/8/3p4/4P3/8/K7 w - - 99 60"                          # e3e4 and e3d4 reset the clock

# the history games of the issue, all tiny
HISTORY_GAMES = [
    (START, SHUFFLE + " " + SHUFFLE),                         # 1: the start identity at plies 0, 4, 8
    (START, ROOKS),                                           # 2: ply 2's placement returns without the rights
    (E5, KNIGHTS_BACK),                                       # 3: en passant counted: not the same identity
    (A5, KNIGHTS_BACK),                                       # 4: not counted: the same identity
    (LONE_EP, SHUFFLE),                                       # 5: a root en-passant square nobody attacks
    ("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq -", "g1f3 e7e5 f3e5"),  # 6: four fields
    (KRK.format(98), "g6g5 h8h7 g5g6"), (KRK.format(99), "g6g5"), (KRK.format(120), "g6g5"),
    (KRK.format(70000), "g6g5 h8h7"), (KRK.format("x"), "g6g5"), (KRK.format("9x"), ""), (KRK.format("-1"), ""),
    (CHESS960, " ".join(R.C960_MOVES.split()[:9])),           # 7: its 7th move castles (the king takes its rook)
]


# ---- a tracker: placement from the host builder, the rest from the move texts ----

def sq_of(text):
    return (ord(text[0]) - 97) | (int(text[1]) - 1) << 3


def root_clock(fen):
    f = fen.split()
    if len(f) < 5 or not f[4].isascii() or not f[4].isdigit():
        return 0
    return min(int(f[4]), 65535)


def root_rights(fen, sqs):
    """The castling field as a set of (colour, rook square)."""
    f = fen.split()
    out = set()
    if len(f) < 3 or f[2] == "-":
        return out
    for ch in f[2]:
        col = 0 if ch.isupper() else 1
        back, rook, king = 56 * col, 4 | col << 3, 6 | col << 3
        ks = [s for s in range(back, back + 8) if sqs[s] == king]
        if not ks:
            continue
        k = ks[0]
        lc = ch.lower()
        if lc == "k":
            cand = [s for s in range(back + 7, k, -1) if sqs[s] == rook]
        elif lc == "q":
            cand = [s for s in range(back, k) if sqs[s] == rook]
        else:
            s = back + ord(lc) - 97
            cand = [s] if sqs[s] == rook else []
        if cand:
            out.add((col, cand[0]))
    return out


def counted_ep(sqs, stm, ep):
    """The en-passant square when a pawn of the side to move attacks it, else None."""
    if ep is None:
        return None
    r = (ep >> 3) + (-1 if stm == 0 else 1)
    own = 1 | stm << 3
    for f in ((ep & 7) - 1, (ep & 7) + 1):
        if 0 <= f < 8 and 0 <= r < 8 and sqs[r * 8 + f] == own:
            return ep
    return None


def track(fen, moves):
    """Per ply of (fen, moves): (identity, clock).  identity = (placement, side to move, rights, counted ep)."""
    ms = moves.split() if isinstance(moves, str) else list(moves)
    recs = F.game_positions(fen, ms)
    f = fen.split()
    sqs = R.squares(recs[0])
    stm = 0 if f[1] == "w" else 1
    rights = root_rights(fen, sqs)
    ep = sq_of(f[3]) if len(f) > 3 and len(f[3]) == 2 and f[3][0] in "abcdefgh" and f[3][1] in "12345678" else None
    clock = root_clock(fen)
    out = [((recs[0][:32].tobytes(), stm, frozenset(rights), counted_ep(sqs, stm, ep)), clock)]
    for i, t in enumerate(ms):
        a, b = sq_of(t[0:2]), sq_of(t[2:4])
        pc, target = int(sqs[a]), int(sqs[b])
        castles = target != 0 and (target >> 3) == stm  # the king takes its own rook
        capture = target != 0 and not castles
        pawn = pc & 7 == 1
        clock = 0 if pawn or capture else min(clock + 1, 65535)
        if pc & 7 == 6:
            rights = {r for r in rights if r[0] != stm}
        rights = {r for r in rights if r[1] not in (a, b)}
        ep = (a + b) // 2 if pawn and abs(a - b) == 16 else None
        stm ^= 1
        sqs = R.squares(recs[i + 1])
        out.append(((recs[i + 1][:32].tobytes(), stm, frozenset(rights), counted_ep(sqs, stm, ep)), clock))
    return out


def tracked_history(games):
    hist, off = [], [0]
    for fen, mv in games:
        t = track(fen, mv)
        for i, (ident, clock) in enumerate(t):
            hist.append((clock, min(sum(1 for q in range(i) if t[q][0] == ident), 255), 0))
        off.append(len(hist))
    return hist, off


def as_tuples(recs, dtype):
    return [tuple(int(r[n]) for n in dtype.names) for r in recs]


# ---- the rule with the DRAW bit, in Python ----

def ends_pv(f):
    return bool(f & (F.END_NO_MOVES | F.END_DRAW))


def mates(f):
    return bool(f & F.END_NO_MOVES) and bool(f & F.END_CHECK)


def reduce_group(ps, po, end, moves):
    """tests/test_search2.py's reduce_group with FNNUE_END_DRAW: a drawn child is worth 0 like a stalemating one."""
    best, key = 0, None
    for c in range(1, len(ps)):
        f = int(end[c])
        if ends_pv(f):
            k = (2, 0) if mates(f) else (1, 0)
        else:
            s = int(ps[c]) + int(po[c])
            k = (1, -(abs(s) // 16 * (1 if s >= 0 else -1)))
        if key is None or k > key:
            best, key = c, k
    if not best:
        return (0, 0, 0, len(ps) - 1, 0, 0, F.BEST_NONE, int(end[0]))
    kind = F.BEST_MATE if key[0] == 2 else F.BEST_CP
    return (R.wrap_neg(ps[best]), R.wrap_neg(po[best]), key[1] if kind == F.BEST_CP else 0, len(ps) - 1, best,
            int(moves[best]) if moves is not None else 0, kind, int(end[0]))


def ordered_children(ps, po, end, moves):
    """fnnue_topk_children's order for one group with the DRAW bit -> LINE_DTYPE tuples, best first."""
    keyed = []
    for c in range(1, len(ps)):
        f = int(end[c])
        if ends_pv(f):
            k = (2, 0) if mates(f) else (1, 0)
        else:
            s = int(ps[c]) + int(po[c])
            k = (1, -(abs(s) // 16 * (1 if s >= 0 else -1)))
        keyed.append((k, c))
    keyed.sort(key=lambda kc: (-kc[0][0], -kc[0][1], kc[1]))
    return [(R.wrap_neg(ps[c]), R.wrap_neg(po[c]), v if r == 1 else 0, c, int(moves[c]) if moves is not None else 0,
             F.BEST_MATE if r == 2 else F.BEST_CP, 0) for (r, v), c in keyed]


def reply_key(f, b):
    if ends_pv(f):
        return (3, 0) if mates(f) else (2, 0)
    if b[BEST["kind"]] == F.BEST_MATE:
        return (1, 0)
    return (2, -b[BEST["value"]])


def reply_rule(end, moves, child_best):
    """tests/test_search2.py's reply_rule with FNNUE_END_DRAW: a drawn child's own record is ignored (but for
    its nodes, and its psqt / positional read as the child's own terms), the pv ends at it, it is worth 0."""
    n = len(end)
    if n == 0:
        return (0,) * 12
    best, key = 0, None
    for c in range(1, n):
        k = reply_key(int(end[c]), child_best[c - 1])
        if key is None or k > key:
            best, key = c, k
    nodes = n - 1 + sum(b[BEST["nodes"]] for b in child_best[:n - 1])
    if not best:
        return (0, 0, 0, nodes, 0, 0, 0, 0, F.BEST_NONE, int(end[0]), 0, 0)
    b = child_best[best - 1]
    mv = int(moves[best]) if moves is not None else 0
    if ends_pv(int(end[best])):
        kind = F.BEST_MATE if key[0] == 3 else F.BEST_CP
        return (R.wrap_neg(b[0]), R.wrap_neg(b[1]), 0, nodes, best, 0, mv, 0, kind, int(end[0]), 1, 0)
    kind = F.BEST_MATED if key[0] == 1 else F.BEST_CP
    return (b[0], b[1], key[1] if kind == F.BEST_CP else 0, nodes, best, b[BEST["best"]], mv, b[BEST["move"]], kind,
            int(end[0]), 2, 0)


def ordered_replies(end, moves, child_best):
    """fnnue_topk_replies' order for one group with the DRAW bit -> LINE2_DTYPE tuples, best first."""
    keyed = [(reply_key(int(end[c]), child_best[c - 1]), c) for c in range(1, len(end))]
    keyed.sort(key=lambda kc: (-kc[0][0], -kc[0][1], kc[1]))
    out = []
    for (rank, value), c in keyed:
        b = child_best[c - 1]
        mv = int(moves[c]) if moves is not None else 0
        kind = M2.CHESS_KIND[rank]
        if ends_pv(int(end[c])):
            out.append((R.wrap_neg(b[0]), R.wrap_neg(b[1]), 0, c, 0, mv, 0, kind, 1, 0))
        else:
            out.append((b[0], b[1], value if kind == F.BEST_CP else 0, c, b[BEST["best"]], mv, b[BEST["move"]], kind,
                        2, 0))
    return out


# ---- the reference of the searches with the draw rules on ----

def drawn(x, history, end):
    """x: (identity, clock) of a searched position; history: the identities before it."""
    if mates(end):
        return False
    return x[1] >= 100 or sum(1 for h in history if h == x[0]) >= 2


def build_reference(data, games):
    """tests/test_search2.py's build_reference with the draw rules on, for the last ply of every game -> per game:
    (search1 tuple, search1 lines best first, search2 tuple, search2 lines best first, drawn children's texts,
    drawn (child, reply) texts)."""
    plies, records = [], []
    for fen, mv in games:
        ms = mv.split()
        c960 = fen == CHESS960
        game = track(fen, ms)
        for q in (len(ms),):
            grp, texts, end = R.expand(fen, ms[:q], c960)
            history = [ident for ident, _ in game[:q + 1]]
            o1 = len(records)
            records.extend(grp)
            kids, marked, marked2 = [], [], []
            for c, t in enumerate(texts):
                x = track(fen, ms[:q] + [t])[-1]
                if drawn(x, history, end[c + 1]):
                    end[c + 1] |= F.END_DRAW
                    marked.append(t)
                g, gt, ge = R.expand(fen, ms[:q] + [t], c960)
                for d, t2 in enumerate(gt):
                    y = track(fen, ms[:q] + [t, t2])[-1]
                    if drawn(y, history + [x[0]], ge[d + 1]):
                        ge[d + 1] |= F.END_DRAW
                        marked2.append((t, t2))
                kids.append((len(records), len(g), gt, ge))
                records.extend(g)
            plies.append((o1, texts, end, kids, marked, marked2))
    ps, po, rc = OracleNet(data).eval_packed(np.array(records, dtype=np.uint8).reshape(-1, 36), threads=8)
    assert rc == 0
    out = []
    for o1, texts, end, kids, marked, marked2 in plies:
        n1 = len(texts) + 1
        codes = [0] + [R.code_of(t) for t in texts]
        one = reduce_group(ps[o1:o1 + n1], po[o1:o1 + n1], end, codes)
        lines1 = ordered_children(ps[o1:o1 + n1], po[o1:o1 + n1], end, codes)
        cb = []
        for c, (o, n, gt, ge) in enumerate(kids):
            if n == 1:  # no legal move: its own terms
                cb.append((int(ps[o]), int(po[o]), 0, 0, 0, 0, F.BEST_NONE, ge[0]))
                continue
            d1 = reduce_group(ps[o:o + n], po[o:o + n], ge, [0] + [R.code_of(x) for x in gt])
            if end[c + 1] & F.END_DRAW:  # a drawn child: its own terms, the rest of its record as it is
                d1 = (int(ps[o]), int(po[o])) + d1[2:]
            cb.append(d1)
        out.append((one, lines1, reply_rule(end, codes, cb), ordered_replies(end, codes, cb), marked, marked2))
    return out


# game 1 cut at plies 5, 6 and 7, and the fifty-move positions: a handful of plies each
G1 = (SHUFFLE + " " + SHUFFLE).split()
DRAW_GAMES = [(START, " ".join(G1[:5])), (START, " ".join(G1[:6])), (START, " ".join(G1[:7])),
              (KRK.format(99), ""), (KRK.format(98), ""), (PAWNS, ""), (KRK.format(120), "")]
I_CUT5, I_CUT6, I_CUT7, I_K99, I_K98, I_PAWNS, I_K120 = range(7)
_REF = {}


def reference():
    """The reference of DRAW_GAMES' last plies on the HD-256 synthetic net: computed once, shared.  (The plies
    before them have nothing drawn below them: the device's records there must equal those without the rules.)"""
    if "r" not in _REF:
        _REF["r"] = build_reference(net_bytes(1, 256, 0), DRAW_GAMES)
    return _REF["r"]


def draw_offsets():
    return np.cumsum([0] + [len(m.split()) + 1 for _, m in DRAW_GAMES])


# ---- the tests ----

def test_layout_and_abi():
    assert F.PLY_HISTORY_DTYPE.itemsize == 4 and N.PLY_HISTORY_BYTES == 4
    assert [(n, F.PLY_HISTORY_DTYPE.fields[n][1]) for n in F.PLY_HISTORY_DTYPE.names] == \
        [("clock", 0), ("seen", 2), ("reserved", 3)]
    assert F.END_DRAW == 0x10 and N.END_DRAW == 0x10
    assert F.END_DRAW & (F.END_NO_MOVES | F.END_CHECK | F.END_EXTINCT | F.END_VARIANT | F.END_WON) == 0
    v = N.lib.fnnue_abi_version()
    assert v >> 16 == 3 and v & 0xFFFF >= 12


def test_new_entry_points_refuse_null_arguments():
    n, g, on = C.c_size_t(), C.c_size_t(), C.c_int()
    L = N.lib
    assert L.fnnue_set_search_draws(None, 1) == E_ARG
    assert L.fnnue_get_search_draws(None, C.byref(on)) == E_ARG
    assert L.fnnue_backend_set_draw_rules(None, 1) == E_ARG
    assert L.fnnue_backend_draw_rules(None, C.byref(on)) == E_ARG
    assert L.fnnue_game_history_device(None, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g), None) == E_ARG
    assert L.fnnue_ctx_game_history(None, b"x", 1, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_game_history(None, 0, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_game_history(b"x", 1, None, None, 1, None, 0, None, 0, None, None) == E_ARG
    assert b"null" in L.fnnue_last_error()
    bad = np.array([0, 9], dtype=np.uint32)
    assert L.fnnue_game_history(b"x", 1, N.ptr(bad), N.ptr(bad), 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG


def test_game_history_capacity_protocol_and_errors():
    text, fo, mo = F.pack_games(HISTORY_GAMES[:2])
    n, g = C.c_size_t(), C.c_size_t()
    rc = N.lib.fnnue_game_history(text, len(text), N.ptr(fo), N.ptr(mo), 2, None, 0, None, 0, C.byref(n), C.byref(g))
    assert rc == -10 and (n.value, g.value) == (9 + 11, 2)
    out = np.zeros(19, dtype=F.PLY_HISTORY_DTYPE)
    off = np.zeros(3, dtype=np.uint32)
    rc = N.lib.fnnue_game_history(text, len(text), N.ptr(fo), N.ptr(mo), 2, N.ptr(out), 19, N.ptr(off), 3,
                                  C.byref(n), C.byref(g))
    assert rc == -10 and (n.value, g.value) == (20, 2)
    for games, code, word in (([(START, "e2e4"), (START, "e2e4 e2e4")], -8, "game 1"), ([("8/8 w - -", "")], -9, "game 0")):
        try:
            F.game_history(games)
            raise AssertionError("not refused")
        except F.FnnueError as err:
            assert err.code == code and word in str(err)
    assert F.game_history([])[1].tolist() == [0]


def test_game_history_against_the_tracker():
    hist, off = F.game_history(HISTORY_GAMES)
    want, woff = tracked_history(HISTORY_GAMES)
    assert off.tolist() == woff
    assert as_tuples(hist, F.PLY_HISTORY_DTYPE) == want
    game = lambda i: hist[off[i]:off[i + 1]]
    # 1: the start identity at plies 0, 4 and 8
    assert game(0)["seen"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2] and game(0)["clock"].tolist() == list(range(9))
    # 2: the placement of ply 2 returns at ply 6 without the king-side rights, then that identity at ply 10
    assert game(1)["seen"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert game(1)["clock"].tolist() == [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    # 3 / 4: en passant counted (another identity) and not counted (the same)
    assert game(2)["seen"].tolist() == [0, 0, 0, 0, 0, 0] and game(3)["seen"].tolist() == [0, 0, 0, 0, 0, 1]
    # 5: the root names e6, nobody attacks it
    assert game(4)["seen"].tolist() == [0, 0, 0, 0, 1] and game(4)["clock"].tolist() == [0, 1, 2, 3, 4]
    # 6: four fields, a capture, and the clock field's forms
    assert game(5)["clock"].tolist() == [0, 1, 0, 0]
    assert [game(i)["clock"].tolist() for i in range(6, 13)] == \
        [[98, 99, 100, 101], [99, 100], [120, 121], [65535, 65535, 65535], [0, 1], [0], [0]]
    # 7: the Chess960 game castles at its 7th move: the clock counts up, the rights go
    c = game(13)
    t = track(*HISTORY_GAMES[13])
    assert R.C960_MOVES.split()[6] == "g1h1" and int(c["clock"][7]) == int(c["clock"][6]) + 1
    assert any(r[0] == 0 for r in t[6][0][2]) and not any(r[0] == 0 for r in t[7][0][2])


def test_rules_with_the_draw_bit_equal_the_old_ones_without_it():
    rnd = np.random.default_rng(5)
    for _ in range(50):
        n = int(rnd.integers(1, 12))
        ps, po = rnd.integers(-3000, 3000, n), rnd.integers(-3000, 3000, n)
        end = rnd.choice([0, 0, 0, 1, 2, 3], n).astype(np.uint8)
        mv = rnd.integers(1, 4096, n)
        assert reduce_group(ps, po, end, mv) == R.reduce_group(ps, po, end, mv)
        cb = [(int(rnd.integers(-9, 9)), 3, int(rnd.integers(-50, 50)), 4, 1, 7, int(rnd.choice([F.BEST_CP, F.BEST_MATE])), 0)
              for _ in range(n - 1)]
        cb = [b if b[6] == F.BEST_CP else b[:2] + (0,) + b[3:] for b in cb]
        assert reply_rule(end, mv, cb) == R.reply_rule(end, mv, cb)
        assert ordered_replies(end, mv, cb) == M2.ordered_lines(end, mv, cb, False)


def test_draw_bit_in_the_rules():
    D, NM, CH = F.END_DRAW, F.END_NO_MOVES, F.END_CHECK
    ps, po = [0, -160, 0, 320], [0, 0, 0, 0]
    # a drawn child ties a 0-valued one: the lower index; with the mate bits beside it: still a mate
    assert reduce_group(ps, po, [0, 0, 0, D], None)[2:5] == (10, 3, 1)
    assert reduce_group([0, 0, 0, 320], po, [0, 0, D, D], None)[2:5] == (0, 3, 1)
    assert reduce_group([0, 0, 0, 320], po, [0, D, 0, D], None)[2:5] == (0, 3, 1)
    assert reduce_group(ps, po, [0, 0, 0, D | NM | CH], None)[6] == F.BEST_MATE
    assert reduce_group(ps, po, [0, 0, 0, D | CH], None)[2:7] == (10, 3, 1, 0, F.BEST_CP)
    kid = lambda kind=F.BEST_CP, value=0, ps=0: (ps, 0, value if kind == F.BEST_CP else 0, 2, 1, 77, kind, 0)
    r = reply_rule([0, D, 0], None, [kid(F.BEST_MATE, ps=5), kid(value=1)])   # the reply would mate: still worth 0
    assert (r[R.B2["best"]], r[R.B2["value"]], r[R.B2["kind"]], r[R.B2["pv_len"]], r[0], r[R.B2["nodes"]]) == \
        (1, 0, F.BEST_CP, 1, -5, 6)
    r = reply_rule([0, 0, D], None, [kid(value=0), kid(value=-900)])          # ties a 0: the lower index
    assert (r[R.B2["best"]], r[R.B2["pv_len"]]) == (1, 2)
    r = reply_rule([0, 0, D | NM | CH], None, [kid(value=-900), kid()])
    assert (r[R.B2["best"]], r[R.B2["kind"]], r[R.B2["pv_len"]]) == (2, F.BEST_MATE, 1)


def test_reference_marks_what_the_issue_says():
    ref = reference()
    last = lambda i: ref[i]
    # ply 7: the child f6g8 is drawn (and below it g1f3, which nobody looks at)
    assert last(I_CUT7)[4] == ["f6g8"] and last(I_CUT7)[5] == [("f6g8", "g1f3")]
    assert last(I_CUT6)[4] == [] and last(I_CUT6)[5] == [("f3g1", "f6g8")]   # ply 6: that grandchild
    assert last(I_CUT5)[4] == [] and last(I_CUT5)[5] == []                   # ply 5: the second occurrence only
    one, lines1, two, lines2, marked, _ = last(I_K99)
    assert (one[BEST["kind"]], F.move_uci(one[BEST["move"]])) == (F.BEST_MATE, "g6h6")
    assert len(marked) == len(lines1) - 1 and all(ln[2] == 0 for ln in lines1[1:])
    assert two[R.B2["kind"]] == F.BEST_MATE and all(ln[8] == 1 and ln[2] == 0 for ln in lines2[1:])
    one, lines1, two, lines2, marked, marked2 = last(I_K98)
    assert marked == [] and len(marked2) > 10 and two[R.B2["kind"]] == F.BEST_MATE
    assert all(ln[2] == 0 for ln in lines2[1:] if ln[8] == 2)                # every quiet reply is worth 0
    _, lines1, _, _, marked, _ = last(I_PAWNS)
    assert sorted(set(F.move_uci(ln[4]) for ln in lines1) - set(marked)) == ["e3d4", "e3e4"]
    _, lines1, _, _, marked, _ = last(I_K120)
    assert len(lines1) > 10 and len(marked) == len(lines1) - 1               # the root is searched, its moves draw

"""Repetition and fifty-move draws in the variant searches, the host side (ABI
3.16): the ABI version, the no-device error paths and the capacity protocol of
the new entry points, F.game_vhistory against a tracker written here (placement
and pockets from F.game_vpositions; rights, en passant, promoted marks and the
clock from the move texts; a move's check from F.game_end's CHECK bit, which
asks the position and not the history), and a host-built reference of the four
variant searches with the rules on (what tests/test_gpu_vdraws.py holds the
device to): records and end bytes from F.game_vchildren / F.game_end, marks from
the tracker, terms from the variant oracle, reductions from the Python rules of
tests/test_vsearch2.py and tests/test_draws.py joined (a drawn record ranks as a
stalemating one; FNNUE_END_WON and a decided end keep precedence)."""
import ctypes as C
import functools

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import VariantOracleNet
from tests import test_draws as D
from tests import test_multipv2 as M2
from tests import test_search2 as R
from tests import test_vsearch2 as V2

ZH, AT, KOTH, RK, TC = (N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL, N.VARIANT_RACINGKINGS,
                        N.VARIANT_THREECHECK)
VARIANTS = (ZH, AT, KOTH, RK, TC)
E_ARG, E_MOVE, E_FEN, E_CAPACITY = -1, -8, -9, -10
CHESS_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
RK_START = "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1"
START = {ZH: ZH_START, AT: CHESS_START, KOTH: CHESS_START, RK: RK_START, TC: CHESS_START}
WON, DRAW, NO_MOVES = F.END_WON, F.END_DRAW, F.END_NO_MOVES
DECIDED = F.END_CHECK | F.END_EXTINCT | F.END_VARIANT
BEST = V2.BEST

# ---- the issue's games ----
SHUFFLE = {v: "g1f3 g8f6 f3g1 f6g8" for v in (ZH, AT, KOTH, TC)}
SHUFFLE[RK] = "e2g3 d2b3 g3e2 b3d2"
ZH_CYCLE = "c3e4 e5e4 N@c3 e4e5 g1h1 N@e4 h1h2 e5d6 h2g1 d6e5"       # a capture and two drops, back at the root
ZH_CAP = ("8/8/8/4k3/4n3/2N5/8/6K1[] w - - 0 1", ZH_CYCLE + " " + ZH_CYCLE)
ZH_POCKET = ("8/8/8/4k3/8/8/8/6K1[N] w - - 0 1", "N@e4 e5e4 g1h1 e4e5 h1h2 e5d6 h2g1 d6e5")  # ply 8: other pockets
QK = "4k3/8/8/8/8/8/8/Q3K3 w - - 0 1"
QK_MOVES = "a1a4 e8e7 a4a1 e7e8 a1a4 e8e7 a4a1 e7e8"
TC_QK = (QK + " +0+0", QK_MOVES)
TC_FIFTH = ("4k3/8/8/8/8/8/8/Q3K3 w - - 3+3 98 60", "a1b1")          # the fifth field holds the counters
KRK = "7k/5K2/6R1/8/8/8/8/8 w - - {} 80"
ZH_KRK = "7k/5K2/6R1/8/8/8/8/8[] w - - {} 80"
RK_99 = "8/8/8/8/8/8/k6K/8 w - - 99 70"


def cut(game, n):
    return (game[0], " ".join(game[1].split()[:n]))


def shuffle_game(v):
    return (START[v], SHUFFLE[v] + " " + SHUFFLE[v])


HISTORY_GAMES = {
    ZH: [shuffle_game(ZH), ZH_CAP, ZH_POCKET, (ZH_KRK.format(99), "g6g5 h8h7"), (ZH_KRK.format(120), "")],
    AT: [shuffle_game(AT)] + [(KRK.format(c), "g6g5 h8h7 g5g6") for c in (99, 98, 120, 70000, "x")] +
        [(CHESS_START, "e2e4 d7d5 e4d5 d8d5 g1f3 d5d2")],            # a pawn capture, then the queen explodes on d2
    KOTH: [shuffle_game(KOTH), (QK, QK_MOVES)] + [(KRK.format(c), "g6g5") for c in (99, 98, 120)],
    RK: [shuffle_game(RK), (RK_99, "h2h3 a2a3")],
    TC: [shuffle_game(TC), (TC_QK[0], QK_MOVES + " a1a4"), TC_FIFTH, (QK + " +1+0", "a1a4 e8e7"),
         ("4k3/8/8/8/8/8/8/Q3K3 w - - 2+3 7 9", "a1a4")],
}

# the searched games: every last ply is held to the reference
DRAW_GAMES = {
    ZH: [cut(shuffle_game(ZH), n) for n in (5, 6, 7)] + [cut(ZH_CAP, n) for n in (8, 9, 18, 19)] +
        [(ZH_KRK.format(99), "")],
    AT: [cut(shuffle_game(AT), n) for n in (5, 6, 7)] + [(KRK.format(c), "") for c in (99, 98, 120)],
    KOTH: [cut(shuffle_game(KOTH), n) for n in (5, 6, 7)] + [((QK, QK_MOVES)[0], " ".join(QK_MOVES.split()[:7]))] +
          [(KRK.format(c), "") for c in (99, 98, 120)],
    RK: [cut(shuffle_game(RK), n) for n in (5, 6, 7)] + [(RK_99, "")],
    TC: [cut(shuffle_game(TC), n) for n in (5, 6, 7)] + [cut(TC_QK, 7), cut(TC_QK, 8)],
}
I_CUT5, I_CUT6, I_CUT7 = 0, 1, 2
I_ZH8, I_ZH9, I_ZH18, I_ZH19, I_ZH_KRK = 3, 4, 5, 6, 7
I_QK7 = 3                      # kingOfTheHill and threeCheck
I_KRK = {AT: (3, 4, 5), KOTH: (4, 5, 6)}  # clocks 99, 98 and 120
I_TC8 = 4
I_RK99 = 3


def net_variant(v):
    return ZH if v == ZH else AT


@functools.lru_cache(maxsize=None)
def net_data(v):
    """The HD-256 nets of tests/test_gpu_vsearch2.py: crazyhouse's own, the atomic one for every other variant."""
    return F.synthesize_variant_net(5, 256, ZH) if v == ZH else F.synthesize_variant_net(6, 256, AT)


# ---- the tracker ----

def fen_fields(fen):
    return fen.split()


def root_clock(v, fen):
    """chess's rule; threeCheck: the first field from the fifth on without a '+'; crazyhouse: no clock."""
    if v == ZH:
        return 0
    f = fen_fields(fen)[4:]
    if v == TC:
        f = [x for x in f if "+" not in x]
    if not f or not f[0].isascii() or not f[0].isdigit():
        return 0
    return min(int(f[0]), 65535)


def root_counters(fen):
    """threeCheck: the checks (white, black) may still give: "3+3" as the fifth field, or a last field "+w+b"."""
    f = fen_fields(fen)[4:]
    if f and len(f[0]) == 3 and f[0][1] == "+":
        return int(f[0][0]), int(f[0][2])
    if f and len(f[-1]) == 4 and f[-1][0] == "+":
        return 3 - int(f[-1][1]), 3 - int(f[-1][3])
    return 3, 3


def root_promoted(fen):
    out, r, f = set(), 7, 0
    for ch in fen_fields(fen)[0]:
        if ch == "[":
            break
        if ch == "/":
            r, f = r - 1, 0
        elif ch.isdigit():
            f += int(ch)
        elif ch == "~":
            out.add(r * 8 + f - 1)
        else:
            f += 1
    return out


def vtrack(v, fen, moves):
    """Per ply of the variant game: (identity, clock).  identity = (placement, side to move, rights, counted en
    passant, then crazyhouse: pockets and promoted marks; threeCheck: both counters)."""
    ms = moves.split() if isinstance(moves, str) else list(moves)
    recs = F.game_vpositions(v, fen, ms)
    f = fen_fields(fen)
    sqs = R.squares(recs[0])
    stm = 0 if f[1] == "w" else 1
    rights = D.root_rights(fen, sqs)
    ep = D.sq_of(f[3]) if len(f) > 3 and len(f[3]) == 2 and f[3][0] in "abcdefgh" and f[3][1] in "12345678" else None
    clock = root_clock(v, fen)
    promoted = root_promoted(fen) if v == ZH else set()
    counters = list(root_counters(fen)) if v == TC else None

    def ident(i, sqs):
        extra = ()
        if v == ZH:
            extra = (recs[i][33:43].tobytes(), frozenset(promoted))
        if v == TC:
            extra = (tuple(counters),)
        return (recs[i][:32].tobytes(), stm, frozenset(rights), D.counted_ep(sqs, stm, ep)) + extra

    out = [(ident(0, sqs), clock)]
    for i, t in enumerate(ms):
        new = R.squares(recs[i + 1])
        if t[1] == "@":  # a drop: no mark, no clock (crazyhouse has none)
            ep = None
        else:
            a, b = D.sq_of(t[0:2]), D.sq_of(t[2:4])
            pc, target = int(sqs[a]), int(sqs[b])
            castles = pc & 7 == 6 and (abs(a - b) == 2 or (target != 0 and (target >> 3) == stm))
            capture = target != 0 and not castles
            pawn = pc & 7 == 1
            clock = 0 if v == ZH or pawn or capture else min(clock + 1, 65535)
            if pc & 7 == 6:
                rights = {r for r in rights if r[0] != stm}
            rights = {r for r in rights if r[1] not in (a, b)}
            # atomic: a rook (or king) that exploded takes its rights along
            rights = {r for r in rights if int(new[r[1]]) == (4 | r[0] << 3) and (6 | r[0] << 3) in new}
            ep = (a + b) // 2 if pawn and abs(a - b) == 16 else None
            if v == ZH:
                assert not castles
                carried = a in promoted
                promoted -= {a, b}
                if pawn and not capture and (a & 7) != (b & 7):
                    promoted.discard(b + (-8 if stm == 0 else 8))  # en passant
                if carried or len(t) > 4:
                    promoted.add(b)
        if v == TC and F.game_end(fen, ms[:i + 1], v) & F.END_CHECK and counters[stm] > 0:
            counters[stm] -= 1
        stm ^= 1
        sqs = new
        out.append((ident(i + 1, sqs), clock))
    return out


def tracked_history(v, games):
    hist, off = [], [0]
    for fen, mv in games:
        t = vtrack(v, fen, mv)
        for i, (ident, clock) in enumerate(t):
            hist.append((clock, min(sum(1 for q in range(i) if t[q][0] == ident), 255), 0))
        off.append(len(hist))
    return hist, off


# ---- the variants' rules with the DRAW bit ----

def ends_pv(f):
    return bool(f & (WON | NO_MOVES | DRAW))


def decided(f):
    return bool(f & WON) or (bool(f & NO_MOVES) and bool(f & DECIDED))


def key1(f, ps, po):
    """A child's (rank, value) in the first reduction: lost at once 0, a decided end 2, else 1 with its value; a
    drawn record is worth 0 like a stalemating one."""
    if f & WON:
        return (0, 0)
    if f & (NO_MOVES | DRAW):
        return (2, 0) if f & NO_MOVES and f & DECIDED else (1, 0)
    s = int(ps) + int(po)
    return (1, -(abs(s) // 16 * (1 if s >= 0 else -1)))


KIND1 = {0: F.BEST_LOST, 1: F.BEST_CP, 2: F.BEST_MATE}


def reduce_group(ps, po, end, moves):
    best, key = 0, None
    for c in range(1, len(ps)):
        k = key1(int(end[c]), ps[c], po[c])
        if key is None or k > key:
            best, key = c, k
    if not best:
        return (0, 0, 0, len(ps) - 1, 0, 0, F.BEST_NONE, int(end[0]))
    kind = KIND1[key[0]]
    return (R.wrap_neg(ps[best]), R.wrap_neg(po[best]), key[1] if kind == F.BEST_CP else 0, len(ps) - 1, best,
            int(moves[best]) if moves is not None else 0, kind, int(end[0]))


def ordered_children(ps, po, end, moves):
    keyed = [(key1(int(end[c]), ps[c], po[c]), c) for c in range(1, len(ps))]
    keyed.sort(key=lambda kc: (-kc[0][0], -kc[0][1], kc[1]))
    return [(R.wrap_neg(ps[c]), R.wrap_neg(po[c]), v if KIND1[r] == F.BEST_CP else 0, c,
             int(moves[c]) if moves is not None else 0, KIND1[r], 0) for (r, v), c in keyed]


def key2(f, b):
    """tests/test_vsearch2.py's child_key with the DRAW bit: a drawn child ranks as one without a legal move."""
    if f & DRAW and not f & WON and not (f & NO_MOVES and f & DECIDED):
        return (2, 0)
    return V2.child_key(f, b)


def reply_rule(end, moves, child_best):
    n = len(end)
    best, key = 0, None
    for c in range(1, n):
        k = key2(int(end[c]), child_best[c - 1])
        if key is None or k > key:
            best, key = c, k
    nodes = n - 1 + sum(b[BEST["nodes"]] for b in child_best[:n - 1])
    if not best:
        return (0, 0, 0, nodes, 0, 0, 0, 0, F.BEST_NONE, int(end[0]), 0, 0)
    b = child_best[best - 1]
    mv = int(moves[best]) if moves is not None else 0
    kind = V2.KIND[key[0]]
    if ends_pv(int(end[best])):
        return (R.wrap_neg(b[0]), R.wrap_neg(b[1]), 0, nodes, best, 0, mv, 0, kind, int(end[0]), 1, 0)
    return (b[0], b[1], key[1] if kind == F.BEST_CP else 0, nodes, best, b[BEST["best"]], mv, b[BEST["move"]], kind,
            int(end[0]), 2, 0)


def ordered_replies(end, moves, child_best):
    keyed = [(key2(int(end[c]), child_best[c - 1]), c) for c in range(1, len(end))]
    keyed.sort(key=lambda kc: (-kc[0][0], -kc[0][1], kc[1]))
    out = []
    for (rank, value), c in keyed:
        b = child_best[c - 1]
        mv = int(moves[c]) if moves is not None else 0
        kind = V2.KIND[rank]
        if ends_pv(int(end[c])):
            out.append((R.wrap_neg(b[0]), R.wrap_neg(b[1]), 0, c, 0, mv, 0, kind, 1, 0))
        else:
            out.append((b[0], b[1], value if kind == F.BEST_CP else 0, c, b[BEST["best"]], mv, b[BEST["move"]], kind,
                        2, 0))
    return out


# ---- the reference ----

def vcode_of(text):
    if text[1] == "@":
        s = D.sq_of(text[2:4])
        return s | s << 6 | " PNBRQ".index(text[0]) << 12
    return R.code_of(text)


def child_texts(v, fen, prefix, grp):
    """The UCI texts of a STAR group's children: found from the squares and pockets that changed and confirmed by
    replaying them.  Records that several moves reach (atomic: two pieces next to the capture square) take their
    texts in the generator's order, by from-square."""
    a = R.squares(grp[0])
    stm = int(grp[0][32])
    own = lambda x: x != 0 and (x >> 3) == stm
    found = {}
    texts = []
    for c in range(1, len(grp)):
        key = grp[c].tobytes()
        if key not in found:
            b = R.squares(grp[c])
            changed = [s for s in range(64) if a[s] != b[s]]
            cands = []
            hand_a, hand_b = grp[0][33 + 5 * stm:38 + 5 * stm], grp[c][33 + 5 * stm:38 + 5 * stm]
            for t in range(5):
                if hand_b[t] < hand_a[t]:
                    cands += ["PNBRQ"[t] + "@" + R.sq_name(s) for s in changed]
            froms = [s for s in changed if own(a[s])] + [s for s in range(64) if a[s] == (6 | stm << 3)]
            for f in dict.fromkeys(froms):
                for t in changed:
                    if t != f:
                        promos = ["q", "r", "b", "n"] if a[f] & 7 == 1 and (t >> 3) in (0, 7) else [""]
                        cands += [R.sq_name(f) + R.sq_name(t) + p for p in promos]
            hits = []
            for text in cands:
                try:
                    last = F.game_vpositions(v, fen, prefix + [text])[-1]
                except F.FnnueError:
                    continue
                if last.tobytes() == key and text not in hits:
                    hits.append(text)
            # castling reached by two spellings: the game's notation is the king's own step unless Chess960
            if len(hits) == 2 and a[D.sq_of(hits[0][0:2])] & 7 == 6 and hits[0][0:2] == hits[1][0:2]:
                hits = [h for h in hits if abs(D.sq_of(h[0:2]) - D.sq_of(h[2:4])) == 2]
            assert hits, (fen, prefix, c)
            found[key] = sorted(hits, key=lambda h: -1 if h[1] == "@" else D.sq_of(h[0:2]))
        texts.append(found[key].pop(0))
    return texts


def vexpand(v, fen, prefix):
    """The last ply of the variant game: its records (ply + children), the children's texts, all end flags."""
    hp, ho = F.game_vchildren(v, fen, prefix)
    grp = hp[int(ho[-2]):int(ho[-1])]
    texts = child_texts(v, fen, prefix, grp)
    end = [F.game_end(fen, prefix, v)] + [F.game_end(fen, prefix + [t], v) for t in texts]
    if v == RK:  # no child here has a king on rank 8: FNNUE_END_WON cannot arise (threeCheck: only from a root)
        assert not any(int(x) & 7 == 6 for g in grp for x in R.squares(g)[56:])
    return grp, texts, end


def drawn(x, history, end):
    """x: (identity, clock) of a searched position; history: the identities before it; never a decided record."""
    if decided(end):
        return False
    return x[1] >= 100 or sum(1 for h in history if h == x[0]) >= 2


def build_reference(v, games):
    """For the last ply of every game of variant v -> (vsearch1 tuple, its lines best first, vsearch2 tuple, its
    lines best first, drawn children's texts, drawn (child, reply) texts, {child text: its depth-1 tuple})."""
    plies, records = [], []
    for fen, mv in games:
        ms = mv.split()
        game = vtrack(v, fen, ms)
        history = [ident for ident, _ in game]
        grp, texts, end = vexpand(v, fen, ms)
        o1 = sum(len(r) for r in records)
        records.append(grp)
        kids, marked, marked2 = [], [], []
        for c, t in enumerate(texts):
            x = vtrack(v, fen, ms + [t])[-1]
            if drawn(x, history, end[c + 1]):
                end[c + 1] |= DRAW
                marked.append(t)
            g, gt, ge = vexpand(v, fen, ms + [t])
            for d, t2 in enumerate(gt):
                y = vtrack(v, fen, ms + [t, t2])[-1]
                if drawn(y, history + [x[0]], ge[d + 1]):
                    ge[d + 1] |= DRAW
                    marked2.append((t, t2))
            kids.append((sum(len(r) for r in records), len(g), gt, ge))
            records.append(g)
        plies.append((o1, texts, end, kids, marked, marked2))
    ps, po, rc = VariantOracleNet(net_data(v), net_variant(v)).eval_packed(np.concatenate(records), threads=8)
    assert rc == 0
    out = []
    for o1, texts, end, kids, marked, marked2 in plies:
        n1 = len(texts) + 1
        codes = [0] + [vcode_of(t) for t in texts]
        one = reduce_group(ps[o1:o1 + n1], po[o1:o1 + n1], end, codes)
        lines1 = ordered_children(ps[o1:o1 + n1], po[o1:o1 + n1], end, codes)
        cb = []
        for c, (o, n, gt, ge) in enumerate(kids):
            if n == 1:  # no legal move: its own terms
                cb.append((int(ps[o]), int(po[o]), 0, 0, 0, 0, F.BEST_NONE, ge[0]))
                continue
            d1 = reduce_group(ps[o:o + n], po[o:o + n], ge, [0] + [vcode_of(x) for x in gt])
            if end[c + 1] & DRAW:  # a drawn child: its own terms, the rest of its record as it is
                d1 = (int(ps[o]), int(po[o])) + d1[2:]
            cb.append(d1)
        out.append((one, lines1, reply_rule(end, codes, cb), ordered_replies(end, codes, cb), marked, marked2,
                    dict(zip(texts, cb))))
    return out


@functools.lru_cache(maxsize=None)
def reference(v):
    """The reference of DRAW_GAMES[v]'s last plies: computed once, shared, never changed."""
    return tuple(build_reference(v, DRAW_GAMES[v]))


# ---- the tests ----

def test_abi_version_and_exports():
    ver = N.lib.fnnue_abi_version()
    assert ver >> 16 == 3 and ver >= (3 << 16) | 16
    assert callable(F.game_vhistory) and hasattr(F.Evaluator, "game_vhistory")
    assert hasattr(F.Evaluator, "set_search_vdraws") and hasattr(F.Evaluator, "search_vdraws")


def test_new_entry_points_refuse_null_arguments():
    n, g, on = C.c_size_t(7), C.c_size_t(7), C.c_int()
    L = N.lib
    assert L.fnnue_set_search_vdraws(None, 1) == E_ARG
    assert L.fnnue_get_search_vdraws(None, C.byref(on)) == E_ARG
    assert L.fnnue_backend_set_variant_draw_rules(None, 1) == E_ARG
    assert L.fnnue_backend_variant_draw_rules(None, C.byref(on)) == E_ARG
    assert L.fnnue_game_vhistory_device(None, AT, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g), None) == E_ARG
    assert L.fnnue_ctx_game_vhistory(None, AT, b"x", 1, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_game_vhistory(AT, None, 0, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_game_vhistory(AT, b"x", 1, None, None, 1, None, 0, None, 0, None, None) == E_ARG
    assert b"null" in L.fnnue_last_error()
    bad = np.array([0, 9], dtype=np.uint32)
    assert L.fnnue_game_vhistory(AT, b"x", 1, N.ptr(bad), N.ptr(bad), 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    for variant in (0, 6, -1):  # chess and unknown variants
        assert L.fnnue_game_vhistory(variant, b"x", 1, N.ptr(bad), N.ptr(bad), 1, None, 0, None, 0, C.byref(n),
                                     C.byref(g)) == E_ARG
        assert b"variant" in L.fnnue_last_error()


def test_game_vhistory_capacity_protocol_and_errors():
    games = HISTORY_GAMES[AT][:2]
    text, fo, mo = F.pack_games(games)
    n, g = C.c_size_t(), C.c_size_t()
    rc = N.lib.fnnue_game_vhistory(AT, text, len(text), N.ptr(fo), N.ptr(mo), 2, None, 0, None, 0, C.byref(n), C.byref(g))
    assert rc == E_CAPACITY and (n.value, g.value) == (9 + 4, 2)
    out = np.zeros(12, dtype=F.PLY_HISTORY_DTYPE)
    off = np.zeros(3, dtype=np.uint32)
    rc = N.lib.fnnue_game_vhistory(AT, text, len(text), N.ptr(fo), N.ptr(mo), 2, N.ptr(out), 12, N.ptr(off), 3,
                                   C.byref(n), C.byref(g))
    assert rc == E_CAPACITY and (n.value, g.value) == (13, 2)
    for v, games, code, word in ((AT, [(CHESS_START, "e2e4"), (CHESS_START, "e2e4 e2e4")], E_MOVE, "game 1"),
                                 (ZH, [("8/8 w - -", "")], E_FEN, "game 0"),
                                 (RK, [(CHESS_START, "")], E_FEN, "game 0")):  # racingKings has no pawns
        try:
            F.game_vhistory(v, games)
            raise AssertionError("not refused")
        except F.FnnueError as err:
            assert err.code == code and word in str(err)
    assert F.game_vhistory(KOTH, [])[1].tolist() == [0]


def test_game_vhistory_against_the_tracker():
    for v in VARIANTS:
        hist, off = F.game_vhistory(v, HISTORY_GAMES[v])
        want, woff = tracked_history(v, HISTORY_GAMES[v])
        assert off.tolist() == woff, v
        assert D.as_tuples(hist, F.PLY_HISTORY_DTYPE) == want, v


def test_game_vhistory_on_the_issues_games():
    game = lambda v, i: (lambda h, o: h[o[i]:o[i + 1]])(*F.game_vhistory(v, HISTORY_GAMES[v]))
    for v in VARIANTS:  # the shuffles: the placement stands at plies 0, 4 and 8
        assert game(v, 0)["seen"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2], v
        assert game(v, 0)["clock"].tolist() == ([0] * 9 if v == ZH else list(range(9))), v
    cap = game(ZH, 1)  # across a capture and two drops: placement and pockets stand at plies 0, 10 and 20
    assert cap["seen"].tolist() == [0] * 10 + [1] * 10 + [2] and not cap["clock"].any()
    pocket = game(ZH, 2)  # ply 8 has ply 0's placement and other pockets
    pos = F.game_vpositions(ZH, *ZH_POCKET)
    assert pos[8][:32].tobytes() == pos[0][:32].tobytes() and pos[8][33:43].tobytes() != pos[0][33:43].tobytes()
    assert not pocket["seen"].any()
    assert not game(ZH, 3)["clock"].any() and not game(ZH, 4)["clock"].any()  # every crazyhouse clock is 0
    assert [game(AT, i)["clock"].tolist() for i in range(1, 6)] == \
        [[99, 100, 101, 102], [98, 99, 100, 101], [120, 121, 122, 123], [65535] * 4, [0, 1, 2, 3]]
    # e4xd5 takes both pawns off, so d8d5 is a quiet move; the queen's explosion on d2 removes pieces
    assert game(AT, 6)["clock"].tolist() == [0, 0, 0, 0, 1, 2, 0]
    qk = game(KOTH, 1)  # kingOfTheHill: the queen's shuffle repeats
    assert qk["seen"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    tc = game(TC, 1)  # threeCheck: the counters differ each time the placement returns
    assert tc["seen"].tolist() == [0] * 10 and tc["clock"].tolist() == list(range(10))
    assert F.game_end(TC_QK[0], QK_MOVES + " a1a4", TC) & F.END_VARIANT
    assert game(TC, 2)["clock"].tolist() == [98, 99]        # "... - 3+3 98 60"
    assert game(TC, 3)["clock"].tolist() == [0, 1, 2]       # "... - 0 1 +1+0"
    assert game(TC, 4)["clock"].tolist() == [7, 8]          # "... - 2+3 7 9"
    assert game(RK, 1)["clock"].tolist() == [99, 100, 101]


def test_rules_equal_the_existing_ones_on_their_inputs():
    rnd = np.random.default_rng(7)
    for _ in range(200):
        n = int(rnd.integers(1, 12))
        ps, po = rnd.integers(-3000, 3000, n), rnd.integers(-3000, 3000, n)
        mv = rnd.integers(1, 4096, n)
        # chess's end bytes with DRAW: tests/test_draws.py's rules
        end = rnd.choice([0, 0, 0, 1, 2, 3, DRAW, DRAW | 2, DRAW | 1, DRAW | 3], n).astype(np.uint8)
        assert reduce_group(ps, po, end, mv) == D.reduce_group(ps, po, end, mv)
        assert ordered_children(ps, po, end, mv) == D.ordered_children(ps, po, end, mv)
        cb = [(int(rnd.integers(-9, 9)), 3, int(rnd.integers(-50, 50)), 4, 1, 7, int(rnd.choice([F.BEST_CP, F.BEST_MATE])), 0)
              for _ in range(n - 1)]
        cb = [b if b[6] == F.BEST_CP else b[:2] + (0,) + b[3:] for b in cb]
        assert reply_rule(end, mv, cb) == D.reply_rule(end, mv, cb)
        assert ordered_replies(end, mv, cb) == D.ordered_replies(end, mv, cb)
        # the variants' end bytes without DRAW: tests/test_vsearch2.py's rule
        vend = rnd.choice([0, 0, 0, 1, 2, 3, 5, 9, 11, WON, WON | 9], n).astype(np.uint8)
        vcb = [V2.kid(int(rnd.choice([F.BEST_CP, F.BEST_CP, F.BEST_MATE, F.BEST_LOST])), int(rnd.integers(-50, 50)),
                      int(rnd.integers(0, 9)), 2, 9, int(rnd.integers(-9, 9)), 4) for _ in range(n - 1)]
        assert reply_rule(vend, mv, vcb) == V2.vreply_rule(vend, mv, vcb)
        assert ordered_replies(vend, mv, vcb) == M2.ordered_lines(vend, mv, vcb, True)
    # DRAW beside the variants' bits: WON and a decided end keep precedence
    k = V2.kid(value=-40)
    assert key2(DRAW, k) == (2, 0) and key2(DRAW | F.END_CHECK, k) == (2, 0) and key2(DRAW | NO_MOVES, k) == (2, 0)
    assert key2(DRAW | WON, k) == (0, 0) and key2(DRAW | NO_MOVES | F.END_EXTINCT, k) == (4, 0)
    assert key1(DRAW, 320, 0) == (1, 0) and key1(DRAW | WON, 320, 0) == (0, 0)
    assert key1(DRAW | NO_MOVES | F.END_VARIANT, 320, 0) == (2, 0)


def test_reference_marks_what_the_issue_says():
    for v in VARIANTS:  # the shuffles, cut as tests/test_draws.py's DRAW_GAMES are
        ref = reference(v)
        back, again = SHUFFLE[v].split()[3], SHUFFLE[v].split()[0]
        assert ref[I_CUT7][4] == [back] and ref[I_CUT7][5] == [(back, again)], v
        assert ref[I_CUT6][4] == [] and ref[I_CUT6][5] == [(SHUFFLE[v].split()[2], back)], v
        assert ref[I_CUT5][4] == [] and ref[I_CUT5][5] == [], v
    zh = reference(ZH)
    # cut at 18: h2g1 d6e5 is ply 20 = 10 = 0; h2h1 d6e5 is ply 16 = 6 once more, a third time as well
    assert zh[I_ZH19][4] == ["d6e5"] and zh[I_ZH18][4] == []
    assert sorted(zh[I_ZH18][5]) == [("h2g1", "d6e5"), ("h2h1", "d6e5")]
    for i in (I_ZH8, I_ZH9, I_ZH_KRK):  # the second occurrence only; no clock in crazyhouse
        assert zh[i][4] == [] and zh[i][5] == [], i
    two = zh[I_ZH19][2]
    assert zh[I_ZH19][6]["d6e5"][:2] != (0, 0) and two[3] == zh[I_ZH19][0][3] + sum(b[3] for b in zh[I_ZH19][6].values())
    # the queen's shuffle: marked under kingOfTheHill, counters apart under threeCheck
    assert reference(KOTH)[I_QK7][4] == ["e7e8"]
    tc = reference(TC)
    assert tc[I_QK7][4] == [] and tc[I_QK7][5] == []
    one, lines1, _, _, marked, _, _ = tc[I_TC8]
    assert (one[BEST["kind"]], F.vmove_uci(one[BEST["move"]])) == (F.BEST_MATE, "a1a4") and "a1a4" not in marked
    # the clocks
    for v in (AT, KOTH):
        i99, i98, i120 = I_KRK[v]
        ref = reference(v)
        one, lines1, two, lines2, marked, marked2, _ = ref[i99]
        quiet = [ln for ln in lines1 if ln[5] == F.BEST_CP]
        assert len(marked) == len(quiet) and all(ln[2] == 0 for ln in quiet), v
        if v == KOTH:  # g6h6 mates and is not drawn: the search answers mate
            assert (one[BEST["kind"]], F.vmove_uci(one[BEST["move"]])) == (F.BEST_MATE, "g6h6") and "g6h6" not in marked
            assert two[8] == F.BEST_MATE and two[10] == 1
        assert ref[i98][4] == [] and len(ref[i98][5]) > 10, v
        assert len(ref[i120][4]) >= len(ref[i120][1]) - 1, v
    rk = reference(RK)[I_RK99]
    assert len(rk[4]) == len(rk[1]) and all(ln[2] == 0 for ln in rk[1])

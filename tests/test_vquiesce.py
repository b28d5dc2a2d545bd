"""The host side of the variants' capture quiescence (ABI 3.15): fnnue_game_vquiet_moves
against fnnue_game_vchildren filtered by "the opponent's pieces on the board decrease" (a
filter that shares nothing with the new generators), the no-device error paths of the new
entry points, the variant material net against the oracle, and the rule of include/fnnue.h
restated in Python: vq_ref, the reference the GPU tests hold fnnue_vquiesce and the variant
searches to.

vq_ref is built from host pieces alone: F.game_vquiet_moves for a node's state, candidates and
move codes, F.vmove_uci for the next node's game text, VariantOracleNet for the two terms,
recursion for the rule.  Every hand-made case first asserts its position's premises with
F.game_end / F.game_vchildren, so a wrong FEN fails loudly."""
import ctypes as C
import functools

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import VariantOracleNet
from tests import vmaterial_net as VM

ZH, AT, KOTH, RK, TC = (N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL, N.VARIANT_RACINGKINGS,
                        N.VARIANT_THREECHECK)
VARIANTS = (ZH, AT, KOTH, RK, TC)
E_ARG, E_ARCH, E_MOVE, E_FEN, E_CAPACITY = -1, -4, -8, -9, -10
MATE = 32000
DOMAIN = MATE - 64
CHESS_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
RK_START = "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1"
START = {ZH: ZH_START, AT: CHESS_START, KOTH: CHESS_START, RK: RK_START, TC: CHESS_START}
OVER = F.VQ_LOST | F.VQ_WON | F.VQ_DRAWN
VALUE = {**VM.VALUE, 6: 0}

# the hand-made positions (the facts asserted of them: test_hand_made_premises)
AT_NXF7 = (CHESS_START, "g1f3 e7e6 f3g5 f8e7")               # g5f7 explodes the black king
AT_OWN_KING = ("4k3/8/8/8/8/8/3p4/3QK3 w - - 0 1", "")       # in check; d1d2 would explode the own king
AT_DEFENDED = ("4k3/8/3p4/4p3/8/8/4Q3/4K3 w - - 0 1", "")    # Qxe5 loses the queen in the explosion
KOTH_HILL = ("8/8/3k4/8/3p4/3K4/8/8 w - - 0 1", "")          # Kxd4 onto the hill
RK_GOAL = ("3n4/3K4/8/8/8/8/8/7k w - - 0 1", "")             # Kxd8 onto rank 8, black cannot catch up
RK_CATCH_UP = ("3n4/3K3k/8/8/8/8/8/8 w - - 0 1", "")         # the same capture, but black can
TC_LAST = ("4k3/5p2/8/7Q/8/8/8/4K3 w - - 1+3 0 1", "")       # Qxf7+ is the last check
TC_TWO = ("4k3/5p2/8/7Q/8/8/8/4K3 w - - 2+3 0 1", "")        # with two to go it is a check like any other
ZH_DROP = ("4r2k/6pp/8/8/8/8/8/K3R3[r] w - - 0 1", "e1e8 r@f8 e8f8")   # Rxe8+ answered by a drop only
ZH_NO_DROP = ("4r2k/6pp/8/8/8/8/8/K3R3[] w - - 0 1", "e1e8")           # with nothing in hand Rxe8 mates
HAND = {
    ZH: [ZH_DROP, ZH_NO_DROP],
    AT: [(AT_NXF7[0], AT_NXF7[1] + " g5f7"), AT_OWN_KING, AT_DEFENDED],
    KOTH: [(KOTH_HILL[0], "d3d4")],
    RK: [(RK_GOAL[0], "d7d8"), (RK_CATCH_UP[0], "d7d8")],
    TC: [(TC_LAST[0], "h5f7"), (TC_TWO[0], "h5f7")],
}
# two short random games per variant that meet captures (test_reference_meets_every_case holds them to it)
SEEDS = {ZH: (11, 12), AT: (21, 22), KOTH: (31, 32), RK: (41, 42), TC: (51, 52)}
PLIES = 24
GAMES = {v: [(START[v], F.random_vgame(s, v, START[v], PLIES)) for s in SEEDS[v]] + HAND[v] for v in VARIANTS}


def net_variant(v: int) -> int:
    """The net that serves variant v: its own for crazyhouse, the atomic one for every other."""
    return ZH if v == ZH else AT


@functools.lru_cache(maxsize=None)
def net_data(v: int, kind: str) -> bytes:
    """The HD-256 nets of the tests: "random" (synthesize_variant_net) or "material"."""
    nv = net_variant(v)
    return F.synthesize_variant_net(5 + nv, 256, nv) if kind == "random" else VM.vmaterial_net(256, nv)


@functools.lru_cache(maxsize=None)
def oracle_of(v: int, kind: str) -> VariantOracleNet:
    return VariantOracleNet(net_data(v, kind), net_variant(v))


def wrap_neg(x):
    return ((-int(x) + 2**31) % 2**32) - 2**31


def trunc16(x: int) -> int:
    return abs(x) // 16 * (1 if x >= 0 else -1)


def neg_decided(v: int) -> int:
    """A decided child value seen from the parent: one ply toward zero, a draw stays a draw."""
    return -(v - 1) if v > 0 else -(v + 1) if v < 0 else 0


# ---- the rule, in Python ----

def vq_ref(oracle, v: int, fen: str, moves: str, d: int, checks: bool, terms=None):
    """Q_d of the variant game's last position -> (psqt, positional, value, nodes, move, len, decided), the
    reported terms oriented to its side to move.  `terms`: its own (psqt, positional) when the caller has them."""
    pos, mv, state = F.game_vquiet_moves(v, fen, moves, checks)
    if state & OVER:
        val = -MATE if state & F.VQ_LOST else MATE if state & F.VQ_WON else 0
        return (0, 16 * val, val, 0, 0, 0, 1)
    chk = bool(state & F.VQ_CHECK)
    if chk and len(pos) == 1:  # mated at every depth
        return (0, -16 * MATE, -MATE, 0, 0, 0, 1)
    if terms is None:
        ps, po, rc = oracle.eval_packed(pos[:1])
        assert rc == 0
        terms = (int(ps[0]), int(po[0]))
    stand = (terms[0], terms[1], trunc16(terms[0] + terms[1]), 0, 0, 0, 0)
    assert abs(stand[2]) < DOMAIN
    if d == 0 or len(pos) == 1:
        return stand
    best = None if chk else stand  # a side in check may not stand pat: candidate 0 is its first evasion
    ps, po, rc = oracle.eval_packed(pos[1:])
    assert rc == 0
    nodes = 0
    for k in range(1, len(pos)):
        ch = vq_ref(oracle, v, fen, (moves + " " + F.vmove_uci(int(mv[k]))).strip(), d - 1, checks,
                    (int(ps[k - 1]), int(po[k - 1])))
        nodes += 1 + ch[3]
        if ch[6]:
            val = neg_decided(ch[2])
            cand = (0, 16 * val, val, 0, int(mv[k]), ch[5] + 1, 1)
        else:
            cand = (wrap_neg(ch[0]), wrap_neg(ch[1]), -ch[2], 0, int(mv[k]), ch[5] + 1, 0)
        if best is None or cand[2] > best[2]:  # strictly greater: the first maximum wins
            best = cand
    return best[:3] + (nodes,) + best[4:]


@functools.lru_cache(maxsize=None)
def reference(v: int, kind: str, d: int, checks: bool):
    """vq_ref of every ply of GAMES[v], game after game: computed once, shared by every test that needs it."""
    o = oracle_of(v, kind)
    return tuple(vq_ref(o, v, fen, " ".join(mv.split()[:q]), d, checks)
                 for fen, mv in GAMES[v] for q in range(len(mv.split()) + 1))


def leaf_terms(q, p: int):
    """The terms a leaf at search depth p takes from its Q: a decided one counts plies from the searched ply,
    a decided draw is (0, 0)."""
    if q[6]:
        val = q[2] - p if q[2] > 0 else q[2] + p if q[2] < 0 else 0
        return 0, 16 * val
    return q[0], q[1]


def quiet_tuples(a):
    return [(int(r["psqt"]), int(r["positional"]), int(r["value"]), int(r["nodes"]), int(r["move"]), int(r["len"]),
             int(r["reserved"])) for r in a]


def pieces(p, colour: int) -> int:
    """The pieces of `colour` on the board of one fnnue_vpos record."""
    sq = np.frombuffer(p.tobytes()[:32], dtype=np.uint8)
    nib = np.concatenate([sq & 15, sq >> 4])
    return int(np.count_nonzero((nib != 0) & ((nib >> 3) == colour)))


def last_group(v, fen, moves):
    pos, off = F.game_vchildren(v, fen, moves)
    return pos[off[-2]:off[-1]]


def uci(v, fen, moves="", checks=True):
    return [F.vmove_uci(int(m)) for m in F.game_vquiet_moves(v, fen, moves, checks)[1][1:]]


# ---- the tests ----

def test_abi_and_constants():
    ver = N.lib.fnnue_abi_version()
    assert ver >> 16 == 3 and ver >= (3 << 16) | 15
    assert (F.VQ_CHECK, F.VQ_LOST, F.VQ_WON, F.VQ_DRAWN) == (1, 2, 4, 8)


def test_new_entry_points_refuse_null_and_bad_arguments():
    n, g, st, d = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
    L = N.lib
    fen = CHESS_START.encode()
    assert L.fnnue_game_vquiet_moves(AT, None, b"", 1, None, 0, None, C.byref(st), C.byref(n)) == E_ARG
    assert L.fnnue_game_vquiet_moves(AT, fen, b"", 1, None, 0, None, None, C.byref(n)) == E_ARG
    assert L.fnnue_game_vquiet_moves(AT, fen, b"", 1, None, 0, None, C.byref(st), None) == E_ARG
    assert b"null" in L.fnnue_last_error()
    assert L.fnnue_game_vquiet_moves(0, fen, b"", 1, None, 0, None, C.byref(st), C.byref(n)) == E_ARG   # chess
    assert L.fnnue_game_vquiet_moves(99, fen, b"", 1, None, 0, None, C.byref(st), C.byref(n)) == E_ARG
    assert L.fnnue_set_search_vquiesce(None, 1, 1) == E_ARG
    assert L.fnnue_get_search_vquiesce(None, C.byref(d), C.byref(st)) == E_ARG
    assert L.fnnue_backend_set_variant_quiesce(None, 1, 1) == E_ARG
    assert L.fnnue_backend_variant_quiesce(None, C.byref(d), C.byref(st)) == E_ARG
    assert L.fnnue_vquiesce_device(None, AT, None, None, None, 1, 1, 1, None, 0, None, 0, C.byref(n), C.byref(g),
                                   None) == E_ARG
    assert L.fnnue_vquiesce(None, AT, b"x", 1, None, None, 1, 1, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG


def test_game_vquiet_moves_capacity_protocol_and_errors():
    n, st = C.c_size_t(), C.c_int()
    fen = AT_OWN_KING[0].encode()   # in check: the position and its three evasions
    assert N.lib.fnnue_game_vquiet_moves(AT, fen, b"", 1, None, 0, None, C.byref(st), C.byref(n)) == E_CAPACITY
    assert n.value == 4 and st.value == F.VQ_CHECK
    out, mv = N.vpositions_array(3), np.zeros(3, dtype=np.uint16)
    assert N.lib.fnnue_game_vquiet_moves(AT, fen, b"", 1, N.ptr(out), 3, N.ptr(mv), C.byref(st),
                                         C.byref(n)) == E_CAPACITY
    assert n.value == 4
    for fen, moves, code in ((CHESS_START, "e2e4 e2e4", E_MOVE), ("8/8 w - -", "", E_FEN)):
        try:
            F.game_vquiet_moves(AT, fen, moves)
            raise AssertionError("not refused")
        except F.FnnueError as err:
            assert err.code == code


def test_game_vquiet_moves_against_filtered_children():
    """Checks off (and any position not in check): the children after which the opponent has fewer pieces on
    the board, in order.  Checks on and in check: every child.  Over: nothing."""
    seen = {"capture": 0, "check": 0, "over": 0, "drop": 0}
    for v in VARIANTS:
        for fen, game in GAMES[v]:
            ms = game.split()
            for q in range(len(ms) + 1):
                moves = " ".join(ms[:q])
                group = last_group(v, fen, moves)
                them = 1 - int(group[0].tobytes()[32])
                before = pieces(group[0], them)
                caps = [k for k in range(1, len(group)) if pieces(group[k], them) < before]
                end = F.game_end(fen, moves, v)
                for checks in (False, True):
                    pos, mv, state = F.game_vquiet_moves(v, fen, moves, checks)
                    assert len(pos) == len(mv) and int(mv[0]) == 0 and all(int(m) for m in mv[1:])
                    assert pos[0].tobytes() == group[0].tobytes()
                    if state & OVER:
                        assert len(pos) == 1 and len(group) == 1 and end & F.END_NO_MOVES, (v, fen, moves)
                        assert bin(state).count("1") == 1
                        seen["over"] += checks
                        continue
                    if state & F.VQ_CHECK:
                        assert checks and v != RK and end & F.END_CHECK
                        assert pos.tobytes() == group.tobytes(), (v, fen, moves)
                        seen["check"] += 1
                        seen["drop"] += any("@" in F.vmove_uci(int(m)) for m in mv[1:])
                    else:
                        assert not checks or v == RK or not end & F.END_CHECK, (v, fen, moves)
                        assert pos[1:].tobytes() == group[caps].tobytes(), (v, fen, moves)
                        seen["capture"] += len(caps)
                    for k in range(1, len(pos)):   # every code replays to its record
                        after = F.game_vpositions(v, fen, (moves + " " + F.vmove_uci(int(mv[k]))).strip())[-1]
                        assert after.tobytes() == pos[k].tobytes()
    assert seen["capture"] > 100 and seen["check"] >= 5 and seen["over"] >= 4 and seen["drop"] >= 1, seen


def test_hand_made_premises():
    """The facts the rule cases below stand on, from fnnue_game_end / fnnue_game_vchildren."""
    END = F.END_NO_MOVES, F.END_CHECK, F.END_EXTINCT, F.END_VARIANT
    assert END == (1, 2, 4, 8)
    assert F.game_end(AT_NXF7[0], AT_NXF7[1] + " g5f7", AT) == 5
    assert F.game_end(*AT_OWN_KING, AT) == F.END_CHECK and len(last_group(AT, *AT_OWN_KING)) == 4
    assert F.game_end(KOTH_HILL[0], "d3d4", KOTH) == 9
    assert F.game_end(RK_GOAL[0], "d7d8", RK) == 9
    assert F.game_end(RK_CATCH_UP[0], "d7d8", RK) == 0 and len(last_group(RK, RK_CATCH_UP[0], "d7d8")) == 6
    assert F.game_end(TC_LAST[0], "h5f7", TC) == 11
    assert F.game_end(TC_TWO[0], "h5f7", TC) == 2 and len(last_group(TC, TC_TWO[0], "h5f7")) == 3
    assert F.game_end(ZH_DROP[0], "e1e8", ZH) == F.END_CHECK
    assert F.game_end(ZH_NO_DROP[0], "e1e8", ZH) == 3
    assert F.game_end(ZH_DROP[0], "e1e8 r@f8 e8f8", ZH) == 3


def test_candidates_of_the_hand_made_positions():
    assert "g5f7" in uci(AT, *AT_NXF7)
    for checks in (False, True):   # d1d2 explodes the own king: no candidate either way
        assert "d1d2" not in uci(AT, *AT_OWN_KING, checks=checks)
    assert uci(AT, *AT_OWN_KING, checks=True) == ["e1f1", "e1e2", "e1f2"]
    assert uci(AT, *AT_OWN_KING, checks=False) == []
    assert uci(ZH, ZH_DROP[0], "e1e8") == ["R@f8", "R@g8"]            # answered by a drop only
    assert uci(ZH, ZH_DROP[0], "e1e8", checks=False) == []
    assert uci(ZH, ZH_NO_DROP[0], "e1e8") == [] and F.game_vquiet_moves(ZH, *ZH_NO_DROP, True)[2] == F.VQ_CHECK
    assert F.game_vquiet_moves(KOTH, KOTH_HILL[0], "d3d4", True)[2] == F.VQ_LOST
    assert F.game_vquiet_moves(RK, RK_GOAL[0], "d7d8", True)[2] == F.VQ_LOST
    assert F.game_vquiet_moves(RK, RK_CATCH_UP[0], "d7d8", True)[2] == 0
    assert F.game_vquiet_moves(TC, TC_LAST[0], "h5f7", True)[2] == F.VQ_LOST
    assert F.game_vquiet_moves(TC, TC_TWO[0], "h5f7", True)[2] == F.VQ_CHECK
    assert F.game_vquiet_moves(TC, "4k3/8/8/8/8/8/8/4K3 w - - 0+3 0 1", "", True)[2] == F.VQ_WON
    assert F.game_vquiet_moves(RK, "3K3k/8/8/8/8/8/8/8 w - - 0 1", "", True)[2] == F.VQ_DRAWN
    assert F.game_vquiet_moves(RK, "3K4/8/8/8/8/8/8/7k w - - 0 1", "", True)[2] == F.VQ_WON


def test_material_net_against_the_oracle():
    for v, games in ((ZH, GAMES[ZH]), (AT, GAMES[AT])):
        o = oracle_of(v, "material")
        for fen, game in games:
            pos = F.game_vpositions(v, fen, game)
            ps, po, rc = o.eval_packed(pos)
            assert rc == 0 and not po.any()
            for p, x in zip(pos, ps):
                raw = p.tobytes()
                sq = np.frombuffer(raw[:32], dtype=np.uint8)
                nib = [int(n) for n in np.concatenate([sq & 15, sq >> 4]) if n]
                if sum(1 for n in nib if n & 7 == 6) < 2:   # a king exploded: (0, 0)
                    assert int(x) == 0
                    continue
                bal = sum(VALUE[n & 7] * (1 if n < 8 else -1) for n in nib)
                bal += sum(VALUE[t + 1] * (raw[33 + t] - raw[38 + t]) for t in range(5))
                assert int(x) == 16 * (bal if raw[32] == 0 else -bal)
    fen = "4r2k/6pp/8/8/8/8/8/K3R3[r] w - - 0 1"
    assert VM.vbalance(fen) == 500 - 500 - 200 - 500
    ps, _, _ = oracle_of(ZH, "material").eval_packed(F.game_vpositions(ZH, fen, ""))
    assert int(ps[0]) == 16 * VM.vbalance(fen)


def test_rule_on_the_atomic_positions():
    o = oracle_of(AT, "material")
    g5f7 = int(F.game_vquiet_moves(AT, *AT_NXF7, True)[1][1 + uci(AT, *AT_NXF7).index("g5f7")])
    for checks in (False, True):   # the capture explodes the king: decided with checks off too
        assert vq_ref(o, AT, *AT_NXF7, 1, checks) == (0, 16 * 31999, 31999, 3, g5f7, 1, 1)
        assert vq_ref(o, AT, AT_NXF7[0], AT_NXF7[1] + " g5f7", 0, checks) == (0, -16 * MATE, -MATE, 0, 0, 0, 1)
    # Qxe5 onto the defended pawn: the queen explodes with it
    stand = VM.vbalance(AT_DEFENDED[0])
    assert stand == 900 - 200
    r = vq_ref(o, AT, *AT_DEFENDED, 2, True)
    after = vq_ref(o, AT, AT_DEFENDED[0], "e2e5", 1, True)
    print("atomic Qxe5: stand pat", stand, "after e2e5 (for black)", after, "decided", r)
    assert uci(AT, *AT_DEFENDED) == ["e2e5"]
    assert -after[2] < stand and r == (16 * stand, 0, stand, 1 + after[3], 0, 0, 0)   # the reference stands pat


def test_rule_on_the_plain_variants_positions():
    for v, (fen, _), move, decided in ((KOTH, KOTH_HILL, "d3d4", True), (RK, RK_GOAL, "d7d8", True),
                                       (RK, RK_CATCH_UP, "d7d8", False), (TC, TC_LAST, "h5f7", True),
                                       (TC, TC_TWO, "h5f7", False)):
        o = oracle_of(v, "material")
        for checks in (False, True):
            r = vq_ref(o, v, fen, "", 1, checks)
            if decided:
                code = int(F.game_vquiet_moves(v, fen, "", checks)[1][1 + uci(v, fen, "", checks).index(move)])
                assert r[:3] == (0, 16 * 31999, 31999) and r[4:] == (code, 1, 1), (v, fen, r)
            else:
                assert r[6] == 0 and abs(r[2]) < DOMAIN, (v, fen, r)


def test_rule_on_the_crazyhouse_drop():
    o = oracle_of(ZH, "material")
    fen = ZH_DROP[0]
    e1e8 = int(F.game_vquiet_moves(ZH, fen, "", True)[1][1])
    assert uci(ZH, fen) == ["e1e8"]
    # nothing in hand: the capture mates with checks on, wins a rook with checks off
    assert vq_ref(o, ZH, ZH_NO_DROP[0], "", 1, True) == (0, 16 * 31999, 31999, 1, e1e8, 1, 1)
    bal = VM.vbalance(ZH_NO_DROP[0])
    assert vq_ref(o, ZH, ZH_NO_DROP[0], "", 1, False) == (16 * (bal + 1000), 0, bal + 1000, 1, e1e8, 1, 0)
    # a rook in hand: the check is answered by a drop only; after r@f8, e8f8 mates, so black drops on g8
    e8f8 = int(F.game_vquiet_moves(ZH, fen, "e1e8 r@f8", True)[1][1])
    assert uci(ZH, fen, "e1e8 r@f8")[0] == "e8f8"
    mate = vq_ref(o, ZH, fen, "e1e8 r@f8", 1, True)
    assert mate == (0, 16 * 31999, 31999, 1, e8f8, 1, 1)
    assert leaf_terms(mate, 1) == (0, 16 * 31998) and leaf_terms(mate, 2) == (0, 16 * 31997)
    first = vq_ref(o, ZH, fen, "e1e8", 1, True)        # no standing pat: candidate 0 is the first evasion
    assert F.vmove_uci(first[4]) == "R@f8" and first[5:] == (1, 0) and first[3] == 2
    r = vq_ref(o, ZH, fen, "e1e8", 2, True)
    assert F.vmove_uci(r[4]) == "R@g8" and r[5:] == (2, 0) and abs(r[2]) < DOMAIN
    assert leaf_terms((0, 0, 0, 0, 0, 0, 1), 2) == (0, 0) and neg_decided(0) == 0


def test_reference_meets_every_case():
    """What the GPU tests rely on the reference to contain (choose other games rather than relax this)."""
    lens, decided, drops = set(), set(), 0
    for v in VARIANTS:
        total = 0
        for d in range(4):
            for checks in (False, True):
                ref = reference(v, "random", d, checks)
                total += sum(r[3] for r in ref)
                lens |= {r[5] for r in ref}
                decided |= {r[6] for r in ref}
                drops += sum(1 for r in ref if r[5] and "@" in F.vmove_uci(r[4]))
                assert all(r[2] == trunc16(r[0] + r[1]) and r[5] <= d and (r[4] == 0) == (r[5] == 0) for r in ref)
        assert 0 < total < 20000, (v, total)
    assert lens == {0, 1, 2, 3} and decided == {0, 1} and drops >= 1

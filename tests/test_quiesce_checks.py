"""The host side of quiescence checks (ABI 3.14): fnnue_game_quiet_moves against
fnnue_game_children / fnnue_game_end (a position in check lists every child)
and against fnnue_game_captures (any other lists its captures), the no-device
error paths of the new entry points, and the rule Q' of include/fnnue.h
restated in Python: qc_ref, the reference the GPU tests hold fnnue_quiesce and
the searches to with the setting on.

qc_ref is built from host pieces alone: F.game_quiet_moves for a node's
candidates, their move codes and the check flag, the oracle for the two terms,
recursion for the rule.  Every rule case first asserts its position's premises
with F.game_end / F.game_children, so a wrong FEN fails loudly."""
import ctypes as C

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet
from tests import material_net as M
from tests import test_quiesce as Q
from tests import test_search2 as R
from tests.positions import CHESS960, START

E_ARG, E_MOVE, E_FEN, E_CAPACITY = -1, -8, -9, -10
MATE = 32000
DOMAIN = MATE - 64

SKEWER = "4k3/8/8/8/8/8/8/r3K2Q w - - 0 1"          # in check from a1, the queen behind the king
CAPTURE_MATE = "r5k1/5ppp/8/8/8/8/8/R3K3 w - - 0 1"  # Rxa8 mates
# the bishop checks, Ke8 / Ke7 walk into the rook, nothing reaches b4: Kg8 is forced, and Rxa8 then mates
CHAIN = "r4k2/5ppp/8/8/1B6/8/8/R3R1K1 b - - 0 1"
RANDOM_GAMES = [(START, F.random_game(seed, START, 24)) for seed in range(1, 13)]


def neg_decided(v: int) -> int:
    """A decided child value seen from the parent: one ply toward zero."""
    return -(v - 1) if v > 0 else -(v + 1)


# ---- the rule, in Python ----

def qc_ref(oracle, fen: str, moves: str, d: int, terms=None, stats=None, inner=False):
    """Q'_d of the game's last position -> (psqt, positional, value, nodes, move, len, decided), the reported
    terms oriented to its side to move.  `terms`: its own (psqt, positional) when the caller has them.
    `stats` (a dict) collects what the reference met: "in_check" nodes that listed evasions, "horizon_mates"
    (mated nodes below the root at remaining depth 0), "max_static" (the largest |s|)."""
    pos, mv, chk = F.game_quiet_moves(fen, moves)
    if chk and len(pos) == 1:  # mated at every depth
        if stats is not None and inner and d == 0:
            stats["horizon_mates"] = stats.get("horizon_mates", 0) + 1
        return (0, -16 * MATE, -MATE, 0, 0, 0, 1)
    if terms is None:
        ps, po, rc = oracle.eval_packed(pos[:1])
        assert rc == 0
        terms = (int(ps[0]), int(po[0]))
    stand = (terms[0], terms[1], Q.trunc16(terms[0] + terms[1]), 0, 0, 0, 0)
    if stats is not None:
        stats["max_static"] = max(stats.get("max_static", 0), abs(stand[2]))
    if d == 0 or len(pos) == 1:
        return stand
    if stats is not None and chk:
        stats["in_check"] = stats.get("in_check", 0) + 1
    best = None if chk else stand  # a side in check may not stand pat: candidate 0 is its first evasion
    ps, po, rc = oracle.eval_packed(pos[1:])
    assert rc == 0
    nodes = 0
    for k in range(1, len(pos)):
        ch = qc_ref(oracle, fen, (moves + " " + F.move_uci(int(mv[k]))).strip(), d - 1,
                    (int(ps[k - 1]), int(po[k - 1])), stats, True)
        nodes += 1 + ch[3]
        if ch[6]:
            v = neg_decided(ch[2])
            cand = (0, 16 * v, v, 0, int(mv[k]), ch[5] + 1, 1)
        else:
            cand = (R.wrap_neg(ch[0]), R.wrap_neg(ch[1]), -ch[2], 0, int(mv[k]), ch[5] + 1, 0)
        if best is None or cand[2] > best[2]:  # strictly greater: the first maximum wins
            best = cand
    return best[:3] + (nodes,) + best[4:]


def quiet_tuples(a):
    return [(int(r["psqt"]), int(r["positional"]), int(r["value"]), int(r["nodes"]), int(r["move"]), int(r["len"]),
             int(r["reserved"])) for r in a]


def leaf_terms(q, p: int):
    """The terms a leaf at search depth p takes from its Q' result: a decided one counts plies from the
    searched ply."""
    if q[6]:
        v = q[2] - p if q[2] > 0 else q[2] + p
        return 0, 16 * v
    return q[0], q[1]


def substituted(oracle, fen, prefix, texts, ps, po, end, d, p):
    """Q.substituted under Q': the terms of one STAR group with every searched leaf's replaced."""
    ps, po = [int(x) for x in ps], [int(x) for x in po]
    for c in range(1, len(ps)):
        if d and not int(end[c]) & (F.END_NO_MOVES | F.END_DRAW):
            ps[c], po[c] = leaf_terms(qc_ref(oracle, fen, " ".join(prefix + [texts[c - 1]]), d, (ps[c], po[c])), p)
    return ps, po


def search_reference(data, games, d, two=True):
    """Q.search_reference with the leaves under Q': the existing reductions over substituted terms, the leaves
    of the one-ply search at p = 1, those of the two-ply search at p = 2."""
    oracle = OracleNet(data)

    def terms(grp):
        ps, po, rc = oracle.eval_packed(np.array(grp, dtype=np.uint8).reshape(-1, 36))
        assert rc == 0
        return ps, po

    out = []
    for fen, mv in games:
        ms, c960 = mv.split(), fen == CHESS960
        for q in range(len(ms) + 1):
            prefix = ms[:q]
            grp, texts, end = R.expand(fen, prefix, c960)
            codes = [0] + [R.code_of(t) for t in texts]
            ps, po = substituted(oracle, fen, prefix, texts, *terms(grp), end, d, 1)
            ply = {"one": R.reduce_group(ps, po, end, codes), "group": (ps, po, end, codes), "texts": texts}
            if two:
                cb = []
                for t in texts:
                    g, gt, ge = R.expand(fen, prefix + [t], c960)
                    gps, gpo = terms(g)
                    if len(g) == 1:  # no legal move: its own terms
                        cb.append((int(gps[0]), int(gpo[0]), 0, 0, 0, 0, F.BEST_NONE, ge[0]))
                    else:
                        gps, gpo = substituted(oracle, fen, prefix + [t], gt, gps, gpo, ge, d, 2)
                        cb.append(R.reduce_group(gps, gpo, ge, [0] + [R.code_of(x) for x in gt]))
                ply["cb"] = cb
                ply["two"] = R.reply_rule(end, codes, cb)
            out.append(ply)
    return out


def children_uci(fen, moves=""):
    """The last ply's legal moves in the order of its children, through the capture / candidate codes' text."""
    pos, off = F.game_children(fen, moves)
    group = pos[off[-2]:off[-1]]
    c960 = fen == CHESS960
    _, texts, _ = R.expand(fen, moves.split(), c960)
    assert len(texts) == len(group) - 1
    return texts


# ---- the tests ----

def test_abi_macros_and_layout():
    v = N.lib.fnnue_abi_version()
    assert v >> 16 == 3 and v >= (3 << 16) | 14
    assert F.VALUE_MATE == MATE and F.QUIET_DECIDED == 1
    assert F.QUIET_DTYPE.names[-1] == "reserved" and F.QUIET_DTYPE.itemsize == 20


def test_new_entry_points_refuse_null_arguments():
    n, on = C.c_size_t(), C.c_int()
    L = N.lib
    assert L.fnnue_set_search_quiesce_checks(None, 1) == E_ARG
    assert L.fnnue_get_search_quiesce_checks(None, C.byref(on)) == E_ARG
    assert L.fnnue_backend_set_quiesce_checks(None, 1) == E_ARG
    assert L.fnnue_backend_quiesce_checks(None, C.byref(on)) == E_ARG
    assert L.fnnue_game_quiet_moves(None, b"", None, 0, None, C.byref(on), C.byref(n)) == E_ARG
    assert L.fnnue_game_quiet_moves(START.encode(), b"", None, 0, None, None, C.byref(n)) == E_ARG
    assert L.fnnue_game_quiet_moves(START.encode(), b"", None, 0, None, C.byref(on), None) == E_ARG
    assert b"null" in L.fnnue_last_error()


def test_game_quiet_moves_capacity_protocol_and_errors():
    n, on = C.c_size_t(), C.c_int()
    fen = SKEWER.encode()   # in check: the position and its three evasions
    assert N.lib.fnnue_game_quiet_moves(fen, b"", None, 0, None, C.byref(on), C.byref(n)) == E_CAPACITY
    assert n.value == 4 and on.value == 1
    out, mv = N.positions_array(3), np.zeros(3, dtype=np.uint16)
    assert N.lib.fnnue_game_quiet_moves(fen, b"", N.ptr(out), 3, N.ptr(mv), C.byref(on), C.byref(n)) == E_CAPACITY
    assert n.value == 4
    for fen, moves, code in ((START, "e2e4 e2e4", E_MOVE), ("8/8 w - -", "", E_FEN)):
        try:
            F.game_quiet_moves(fen, moves)
            raise AssertionError("not refused")
        except F.FnnueError as err:
            assert err.code == code


def test_game_quiet_moves_against_children_and_captures():
    plies = [(fen, " ".join(moves.split()[:i])) for fen, moves in RANDOM_GAMES + R.GAMES
             for i in range(len(moves.split()) + 1)]
    hand = Q.HAND_MADE + [(SKEWER, ""), (CAPTURE_MATE, ""), (CAPTURE_MATE, "a1a8"), (CHAIN, ""), (R.MATED, "")]
    checks = quiet = 0
    for fen, moves in plies + hand:
        pos, mv, chk = F.game_quiet_moves(fen, moves)
        assert chk == bool(F.game_end(fen, moves) & F.END_CHECK), (fen, moves)
        assert len(pos) == len(mv) and int(mv[0]) == 0 and all(int(m) for m in mv[1:])
        if chk:   # every child, in order
            kids, off = F.game_children(fen, moves)
            group = kids[off[-2]:off[-1]]
            assert pos.tobytes() == group.tobytes(), (fen, moves)
            checks += 1
        else:     # the captures, unchanged
            cpos, cmv = F.game_captures(fen, moves)
            assert pos.tobytes() == cpos.tobytes() and mv.tobytes() == cmv.tobytes(), (fen, moves)
            quiet += 1
        for k in range(1, len(pos)):   # every code replays to its record
            after = F.game_positions(fen, (moves + " " + F.move_uci(int(mv[k]))).strip())[-1]
            assert after.tobytes() == pos[k].tobytes()
    assert checks >= 5 and quiet > 200    # four hand-made positions in check, and at least one from the games
    uci = lambda fen, moves="": [F.move_uci(int(m)) for m in F.game_quiet_moves(fen, moves)[1][1:]]
    assert uci(Q.IN_CHECK) == children_uci(Q.IN_CHECK) and "g2f3" in uci(Q.IN_CHECK) and len(uci(Q.IN_CHECK)) > 1
    assert uci(CAPTURE_MATE, "a1a8") == [] and F.game_quiet_moves(CAPTURE_MATE, "a1a8")[2]
    assert uci(START) == [] and not F.game_quiet_moves(START)[2]


def test_rule_on_the_skewer():
    o = Q.material_oracle()
    kids = children_uci(SKEWER)
    assert F.game_end(SKEWER) == F.END_CHECK                       # in check, with moves
    assert kids == ["e1d2", "e1e2", "e1f2"]                        # the king steps off the rank
    assert len(F.game_captures(SKEWER)[0]) == 1                    # and no capture
    bal = M.balance(SKEWER)
    assert bal == 400
    # the plain rule stands pat a queen for a rook ahead
    assert Q.q_ref(o, SKEWER, "", 2) == (16 * bal, 0, bal, 0, 0, 0)
    r = qc_ref(o, SKEWER, "", 2)
    first, second = F.game_quiet_moves(SKEWER)[1][1], R.code_of("a1h1")
    assert F.move_uci(int(first)) == kids[0]
    assert r[2] == bal - 900 and r[4] == int(first) and r[5] == 2 and r[6] == 0
    assert r[:2] == (16 * (bal - 900), 0)
    # the line's second move takes the queen
    reply = qc_ref(o, SKEWER, kids[0], 1)
    assert reply[4] == second and reply[2] == 900 - bal
    assert r[3] == sum(1 + qc_ref(o, SKEWER, k, 1)[3] for k in kids) and r[3] > len(kids)
    # at the horizon a side in check that has a move stands pat: both rules agree
    assert qc_ref(o, SKEWER, "", 0) == Q.q_ref(o, SKEWER, "", 0) + (0,)


def test_rule_on_the_capture_that_mates():
    o = Q.material_oracle()
    assert F.game_end(CAPTURE_MATE) == 0
    assert F.game_end(CAPTURE_MATE, "a1a8") == F.END_NO_MOVES | F.END_CHECK
    a1a8 = R.code_of("a1a8")
    assert [int(m) for m in F.game_captures(CAPTURE_MATE)[1][1:]] == [a1a8]
    assert qc_ref(o, CAPTURE_MATE, "", 1) == (0, 16 * 31999, 31999, 1, a1a8, 1, 1)
    assert qc_ref(o, CAPTURE_MATE, "", 3) == (0, 16 * 31999, 31999, 1, a1a8, 1, 1)
    bal = M.balance(CAPTURE_MATE)
    assert Q.q_ref(o, CAPTURE_MATE, "", 1) == (16 * (bal + 500), 0, bal + 500, 1, a1a8, 1)   # "a rook won"
    assert qc_ref(o, CAPTURE_MATE, "", 0) == (16 * bal, 0, bal, 0, 0, 0, 0)
    # the mated position itself, at every depth
    for d in range(3):
        assert qc_ref(o, CAPTURE_MATE, "a1a8", d) == (0, -16 * MATE, -MATE, 0, 0, 0, 1)


def test_rule_on_the_distance_chain():
    o = Q.material_oracle()
    assert F.game_end(CHAIN) == F.END_CHECK
    assert children_uci(CHAIN) == ["f8g8"]                                   # the evasion is forced
    assert F.game_end(CHAIN, "f8g8") == 0
    assert F.game_end(CHAIN, "f8g8 a1a8") == F.END_NO_MOVES | F.END_CHECK    # and the capture mates
    f8g8, a1a8 = R.code_of("f8g8"), R.code_of("a1a8")
    assert qc_ref(o, CHAIN, "f8g8 a1a8", 0)[2] == -32000
    assert qc_ref(o, CHAIN, "f8g8", 1) == (0, 16 * 31999, 31999, 1, a1a8, 1, 1)
    assert qc_ref(o, CHAIN, "", 2) == (0, 16 * -31998, -31998, 2, f8g8, 2, 1)
    assert qc_ref(o, CHAIN, "", 3) == (0, 16 * -31998, -31998, 2, f8g8, 2, 1)
    # one level short of the mate: the forced evasion's own static value, no standing pat for the side in check
    bal = M.balance(CHAIN)
    assert qc_ref(o, CHAIN, "", 1) == (16 * bal, 0, bal, 1, f8g8, 1, 0)
    assert neg_decided(-32000) == 31999 and neg_decided(31999) == -31998 and neg_decided(-31998) == 31997
    # in a search, a leaf at depth p counts its plies from the searched ply
    assert leaf_terms(qc_ref(o, CHAIN, "f8g8", 1), 1) == (0, 16 * 31998)
    assert leaf_terms(qc_ref(o, CHAIN, "", 2), 2) == (0, 16 * -31996)


def test_nets_stay_inside_the_static_domain():
    """The premise of the rule's mate values: |s| < FNNUE_VALUE_MATE - 64 on every static value the reference
    meets, on the material net and on the random HD-256 net."""
    games = RANDOM_GAMES[:3] + Q.HAND_MADE + [(SKEWER, ""), (CAPTURE_MATE, ""), (CHAIN, "")]
    for data in (M.material_net(128), R.net_bytes(1, 256, 0)):
        o, stats = OracleNet(data), {}
        for fen, moves in games:
            ms = moves.split()
            for q in range(0, len(ms) + 1, 4):
                r = qc_ref(o, fen, " ".join(ms[:q]), 2, stats=stats)
                assert r[2] == Q.trunc16(r[0] + r[1]) and r[5] <= 2 and (r[4] == 0) == (r[5] == 0)
        assert 0 < stats["max_static"] < DOMAIN - 64, stats


def test_reference_one_ply_sees_the_mate_behind_the_capture():
    data = M.material_net(128)
    fen = "6k1/5ppp/r7/8/8/8/8/R3K3 b - - 0 1"
    assert "a6a8" in children_uci(fen) and F.game_end(fen, "a6a8 a1a8") == F.END_NO_MOVES | F.END_CHECK
    ply = search_reference(data, [(fen, "")], 1, two=False)[0]
    c = 1 + ply["texts"].index("a6a8")
    assert (ply["group"][0][c], ply["group"][1][c]) == (0, 16 * 31998)   # the leaf, p = 1, the mate one ply below
    plain = Q.search_reference(data, [(fen, "")], 1, two=False)[0]
    assert plain["group"][0][c] == 16 * M.balance(CAPTURE_MATE) + 16 * 500
    # the best move avoids it under both rules here; its value is a material one
    assert abs(ply["one"][R.BEST["value"]]) < DOMAIN

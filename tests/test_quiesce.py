"""The host side of capture quiescence (ABI 3.13): the layout of fnnue_quiet,
the no-device error paths of the new entry points, fnnue_game_captures against
fnnue_game_children filtered by piece count, the material net against the
oracle, and the rule of include/fnnue.h restated in Python: q_ref, the
reference the GPU tests hold fnnue_quiesce and the searches to.

q_ref is built from host pieces alone: F.game_captures for a node's captures
and their move codes, the oracle for the two terms, recursion for the rule."""
import ctypes as C

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet
from tests import material_net as M
from tests import test_search2 as R
from tests.positions import CHESS960, START

E_ARG, E_MOVE, E_FEN, E_CAPACITY = -1, -8, -9, -10

HANGS = "4k3/8/3p4/4p3/8/8/4Q3/4K3 w - - 0 1"     # Qxe5 wins a pawn and loses the queen to dxe5
TRADE = "4k3/8/3p4/4r3/8/8/4R3/4K3 w - - 0 1"     # Rxe5 dxe5: the balance stays -100, standing pat wins the tie
EP = ("4k3/3p4/8/4P3/8/8/8/4K3 b - - 0 1", "d7d5")            # e5xd6 en passant
EP_NOBODY = "4k3/8/8/3p4/8/8/8/4K3 w - d6 0 1"                # an en-passant square nobody can take
PROMO = "3r3k/4P3/8/8/8/8/8/4K3 w - - 0 1"                    # e7xd8 = Q, R, B, N (and the quiet e8 promotions)
PINNED = "4r2k/8/8/8/8/3p4/4N3/4K3 w - - 0 1"                 # Nxd3 would leave the king to the rook
IN_CHECK = "4k3/8/8/8/8/2p2n2/3P2P1/4K2R w - - 0 1"           # Nf3 checks: gxf3 answers it, dxc3 does not
BARE = "4k3/8/8/8/8/8/8/4K3 w - - 0 1"
KQK = "4k3/8/8/8/8/8/8/3QK3 w - - 0 1"
HAND_MADE = [(HANGS, ""), (TRADE, ""), EP, (EP_NOBODY, ""), (PROMO, ""), (PINNED, ""), (IN_CHECK, ""),
             (CHESS960, " ".join(R.C960_MOVES.split()[:6])), (BARE, ""), (KQK, "")]


def trunc16(s: int) -> int:
    return abs(s) // 16 * (1 if s >= 0 else -1)


def pieces(rec) -> int:
    return int(np.count_nonzero(R.squares(rec)))


def captures_by_children(fen: str, moves: str):
    """The last ply's children with one piece fewer than the ply, in order: what game_captures must return."""
    pos, off = F.game_children(fen, moves)
    group = pos[off[-2]:off[-1]]
    return [group[0]] + [c for c in group[1:] if pieces(c) == pieces(group[0]) - 1]


# ---- the rule, in Python ----

def q_ref(oracle, fen: str, moves: str, d: int, terms=None):
    """Q_d of the game's last position -> (psqt, positional, value, nodes, move, len), the reported terms
    oriented to its side to move.  `terms`: its own (psqt, positional) when the caller has them."""
    pos, mv = F.game_captures(fen, moves)
    if terms is None:
        ps, po, rc = oracle.eval_packed(pos[:1])
        assert rc == 0
        terms = (int(ps[0]), int(po[0]))
    best = (terms[0], terms[1], trunc16(terms[0] + terms[1]), 0, 0, 0)  # candidate 0: standing pat
    if d == 0 or len(pos) == 1:
        return best
    ps, po, rc = oracle.eval_packed(pos[1:])
    assert rc == 0
    nodes = 0
    for k in range(1, len(pos)):
        ch = q_ref(oracle, fen, (moves + " " + F.move_uci(int(mv[k]))).strip(), d - 1, (int(ps[k - 1]), int(po[k - 1])))
        nodes += 1 + ch[3]
        if -ch[2] > best[2]:  # strictly greater: the first maximum wins
            best = (R.wrap_neg(ch[0]), R.wrap_neg(ch[1]), -ch[2], 0, int(mv[k]), ch[5] + 1)
    return best[:3] + (nodes,) + best[4:]


QUIET = dict(zip(("psqt", "positional", "value", "nodes", "move", "len"), range(6)))


def quiet_tuples(a):
    return [(int(r["psqt"]), int(r["positional"]), int(r["value"]), int(r["nodes"]), int(r["move"]), int(r["len"]))
            for r in a]


_MATERIAL = {}


def material_oracle():
    if "o" not in _MATERIAL:
        _MATERIAL["o"] = OracleNet(M.material_net(128))
    return _MATERIAL["o"]


# ---- the tests ----

def test_layout_and_abi():
    assert F.QUIET_DTYPE.itemsize == 20
    assert [(n, F.QUIET_DTYPE.fields[n][1]) for n in F.QUIET_DTYPE.names] == \
        [("psqt", 0), ("positional", 4), ("value", 8), ("nodes", 12), ("move", 16), ("len", 18), ("reserved", 19)]
    assert F.QUIESCE_MAX == 4
    v = N.lib.fnnue_abi_version()
    assert v >> 16 == 3 and v >= (3 << 16) | 13


def test_new_entry_points_refuse_null_arguments():
    n, g, d, sl = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_uint64()
    L = N.lib
    assert L.fnnue_set_search_quiesce(None, 1) == E_ARG
    assert L.fnnue_get_search_quiesce(None, C.byref(d)) == E_ARG
    assert L.fnnue_quiesce_slices(None, C.byref(sl)) == E_ARG
    assert L.fnnue_backend_set_quiesce(None, 1) == E_ARG
    assert L.fnnue_backend_quiesce(None, C.byref(d)) == E_ARG
    assert L.fnnue_quiesce_device(None, None, None, None, 1, 1, None, 0, None, 0, C.byref(n), C.byref(g), None) == E_ARG
    assert L.fnnue_quiesce(None, b"x", 1, None, None, 1, 5, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_game_captures(None, b"", None, 0, None, C.byref(n)) == E_ARG
    assert L.fnnue_game_captures(START.encode(), b"", None, 0, None, None) == E_ARG
    assert b"null" in L.fnnue_last_error()


def test_game_captures_capacity_protocol_and_errors():
    n = C.c_size_t()
    fen = PROMO.encode()
    assert N.lib.fnnue_game_captures(fen, b"", None, 0, None, C.byref(n)) == E_CAPACITY and n.value == 5
    out, mv = N.positions_array(4), np.zeros(4, dtype=np.uint16)
    assert N.lib.fnnue_game_captures(fen, b"", N.ptr(out), 4, N.ptr(mv), C.byref(n)) == E_CAPACITY and n.value == 5
    for fen, moves, code in ((START, "e2e4 e2e4", E_MOVE), ("8/8 w - -", "", E_FEN)):
        try:
            F.game_captures(fen, moves)
            raise AssertionError("not refused")
        except F.FnnueError as err:
            assert err.code == code


def test_game_captures_against_the_children_filtered_by_piece_count():
    plies = [(fen, " ".join(moves.split()[:i])) for fen, moves in R.GAMES for i in range(len(moves.split()) + 1)]
    seen = 0
    for fen, moves in plies + HAND_MADE:
        pos, mv = F.game_captures(fen, moves)
        want = captures_by_children(fen, moves)
        assert len(pos) == len(want) == len(mv) and pos.tobytes() == np.array(want).tobytes(), (fen, moves)
        assert int(mv[0]) == 0 and all(int(m) for m in mv[1:])
        # every code replays to its record
        for k in range(1, len(pos)):
            after = F.game_positions(fen, (moves + " " + F.move_uci(int(mv[k]))).strip())[-1]
            assert after.tobytes() == pos[k].tobytes()
        seen += len(pos) - 1
    assert seen > 20
    uci = lambda fen, moves="": [F.move_uci(int(m)) for m in F.game_captures(fen, moves)[1][1:]]
    assert uci(*EP) == ["e5d6"]
    assert uci(EP_NOBODY) == []
    assert uci(PROMO) == ["e7d8q", "e7d8r", "e7d8b", "e7d8n"]
    assert uci(PINNED) == []
    assert uci(IN_CHECK) == ["g2f3"]
    assert uci(BARE) == [] and uci(START) == []
    # the Chess960 game's 7th move castles, spelled king takes own rook: a legal move, and no capture
    c960 = " ".join(R.C960_MOVES.split()[:6])
    assert R.C960_MOVES.split()[6] == "g1h1" and "g1h1" not in uci(CHESS960, c960)
    kids, off = F.game_children(CHESS960, c960)
    assert any(np.array_equal(k, F.game_positions(CHESS960, c960 + " g1h1")[-1]) for k in kids[off[-2] + 1:off[-1]])


def test_material_net_counts_material():
    o = material_oracle()
    fens = [START, HANGS, TRADE, EP[0], EP_NOBODY, PROMO, PINNED, IN_CHECK, BARE, KQK, R.MANY, R.MATED,
            "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R b KQkq - 2 2",
            "8/5k2/8/8/2q5/8/1R6/K7 b - - 0 1"]
    pos = np.stack([F.pos_from_fen(f) for f in fens])
    ps, po, rc = o.eval_packed(pos)
    assert rc == 0 and not po.any()
    assert [trunc16(int(p)) for p in ps] == [M.balance(f) for f in fens]
    assert ps.tolist() == [16 * M.balance(f) for f in fens]
    assert M.balance(HANGS) == 700 and M.balance("8/5k2/8/8/2q5/8/1R6/K7 b - - 0 1") == 400


def test_rule_on_the_hanging_queen():
    o = material_oracle()
    e2e5 = next(int(m) for m in F.game_captures(HANGS)[1][1:])
    assert F.move_uci(e2e5) == "e2e5"
    assert q_ref(o, HANGS, "", 0) == (16 * 700, 0, 700, 0, 0, 0)
    # one capture deep the pawn looks free: +100 over standing pat, the terms those of the line's end, negated
    assert q_ref(o, HANGS, "", 1) == (16 * 800, 0, 800, 1, e2e5, 1)
    # two deep dxe5 answers: standing pat; the tree holds Qxe5 and dxe5
    assert q_ref(o, HANGS, "", 2) == (16 * 700, 0, 700, 2, 0, 0)
    assert q_ref(o, HANGS, "", 4) == (16 * 700, 0, 700, 2, 0, 0)   # the tree ends before the depth does
    # from the other side, after Qxe5: the recapture wins the queen
    assert q_ref(o, HANGS, "e2e5", 1)[2:] == (100, 1, F.game_captures(HANGS, "e2e5")[1][1], 1)


def test_rule_on_an_equal_trade_stands_pat():
    o = material_oracle()
    assert q_ref(o, TRADE, "", 1)[QUIET["value"]] == 400
    r = q_ref(o, TRADE, "", 2)
    assert r == (16 * -100, 0, -100, 2, 0, 0)   # Rxe5 dxe5 is worth -100 as well: the first maximum is standing pat


def test_rule_on_a_random_net_keeps_the_triple_consistent():
    o = OracleNet(R.net_bytes(1, 256, 0))
    for fen, moves in HAND_MADE:
        for d in range(4):
            ps, po, v, nodes, mv, ln = q_ref(o, fen, moves, d)
            assert v == trunc16(ps + po) and ln <= d and (mv == 0) == (ln == 0)
            assert (nodes == 0) == (d == 0 or len(F.game_captures(fen, moves)[0]) == 1)


# ---- the searches' reference: host replays, the oracle's terms, q_ref for the leaves, the rules ----

FLIP = "3r3k/8/8/8/3N4/2P5/8/K7 w - - 0 1"   # ...Rxd4 wins a defended knight, and cxd4 takes the rook back


def substituted(oracle, fen, prefix, texts, ps, po, end, d):
    """The terms of one STAR group with every leaf's replaced by the reported terms of Q_d (records j >= 1
    whose end byte has neither NO_MOVES nor DRAW)."""
    ps, po = [int(x) for x in ps], [int(x) for x in po]
    for c in range(1, len(ps)):
        if d and not int(end[c]) & (F.END_NO_MOVES | F.END_DRAW):
            q = q_ref(oracle, fen, " ".join(prefix + [texts[c - 1]]), d, (ps[c], po[c]))
            ps[c], po[c] = q[0], q[1]
    return ps, po


def search_reference(data, games, d, reduce_group=R.reduce_group, reply_rule=R.reply_rule, two=True):
    """Per ply in game order: {"one": the fnnue_best tuple, "group": (ps, po, end, codes) with the substituted
    terms, "two": the fnnue_best2 tuple, "cb": the children's depth-1 tuples, "texts": the children's moves}."""
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
            ps, po = substituted(oracle, fen, prefix, texts, *terms(grp), end, d)
            ply = {"one": reduce_group(ps, po, end, codes), "group": (ps, po, end, codes), "texts": texts}
            if two:
                cb = []
                for t in texts:
                    g, gt, ge = R.expand(fen, prefix + [t], c960)
                    gps, gpo = terms(g)
                    if len(g) == 1:  # no legal move: its own terms
                        cb.append((int(gps[0]), int(gpo[0]), 0, 0, 0, 0, F.BEST_NONE, ge[0]))
                    else:
                        gps, gpo = substituted(oracle, fen, prefix + [t], gt, gps, gpo, ge, d)
                        cb.append(reduce_group(gps, gpo, ge, [0] + [R.code_of(x) for x in gt]))
                ply["cb"] = cb
                ply["two"] = reply_rule(end, codes, cb)
            out.append(ply)
    return out


def test_reference_one_ply_on_the_hanging_queen():
    data = M.material_net(128)
    off0 = search_reference(data, [(HANGS, "")], 0, two=False)[0]["one"]
    on1 = search_reference(data, [(HANGS, "")], 1, two=False)[0]["one"]
    assert F.move_uci(off0[R.BEST["move"]]) == "e2e5" and off0[R.BEST["value"]] == 800
    assert F.move_uci(on1[R.BEST["move"]]) != "e2e5" and on1[R.BEST["value"]] == 700
    assert off0[R.BEST["nodes"]] == on1[R.BEST["nodes"]]


def test_reference_two_plies_the_reply_that_hangs_a_rook():
    data = M.material_net(128)
    off0 = search_reference(data, [(FLIP, "")], 0)[0]["two"]
    on2 = search_reference(data, [(FLIP, "")], 2)[0]["two"]
    # static leaves: every move that leaves the knight on d4 loses it to Rxd4; the first knight move is best
    assert (F.move_uci(off0[R.B2["move"]]), off0[R.B2["value"]]) == ("d4c2", -100)
    # resolved leaves: Rxd4 cxd4 loses the rook, nothing is threatened, and the first move of all is as good
    assert (F.move_uci(on2[R.B2["move"]]), on2[R.B2["value"]]) == ("a1b1", -100)
    assert off0[R.B2["nodes"]] == on2[R.B2["nodes"]]

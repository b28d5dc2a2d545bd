"""The host side of the two-ply search (ABI 3.7): the layout of fnnue_best2,
the no-device error paths of the new entry points, the `analysis` JSON with a
two-move pv, and the reference the GPU tests hold fnnue_search2 to.

The reference is built from host pieces alone: F.game_children for a ply's
children and a child's own children, F.game_positions / F.game_end for move
texts and end flags, the oracle for the two terms, and the rule of
include/fnnue.h restated in Python below."""
import ctypes as C
import json
import os

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from oracle.oracle import OracleNet
from tests.conftest import ROOT, net_bytes
from tests.positions import CHESS960, START

E_ARG = -1
WCC = json.load(open(os.path.join(ROOT, "tests", "golden", "wcc_games.json")))["games"]
MANY = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"  # 218 legal moves
MATE_OR_STALEMATE = "7k/5Q2/5K2/8/8/8/8/8 w - - 0 1"            # Qg7 / Qf8 mate, Kg6 stalemates
FOOLS_MATE = "f2f3 e7e5 g2g4 d8h4"
C960_MOVES = F.random_game(15, CHESS960, 30)                    # its 7th move, g1h1, castles (king takes rook)
MATED = "8/8/8/1P6/8/6k1/r7/7K w - - 0 1"                        # b6 and Kg1 both allow Ra1#

# ~45 plies, ~25k grandchildren
GAMES = [(g["position"], " ".join(g["moves"].split()[:9])) for g in WCC[:2]]   # 10 plies each
GAMES += [(CHESS960, " ".join(C960_MOVES.split()[:7])),                         # up to its castling move
          (MANY, ""), (MATE_OR_STALEMATE, ""),
          (START, "f2f3 e7e5 g2g4"),   # a mate in one is there
          (START, "f2f3 e7e5"),        # g2g4 allows it: that child ranks last
          (MATED, ""),                 # every move allows a mate in one
          (START, FOOLS_MATE)]         # a finished game
I_C960, I_MANY, I_MOS, I_MATE1, I_BLUNDER, I_MATED, I_FINISHED = 2, 3, 4, 5, 6, 7, 8


# ---- the rule, in Python ----

def wrap_neg(x):
    return ((-int(x) + 2**31) % 2**32) - 2**31


def reduce_group(ps, po, end, moves):
    """fnnue_best_children for one group (record 0 = the parent), test_gpu_search1's
    reduce_groups pattern: (psqt, positional, value, nodes, best, move, kind, end)."""
    best, key = 0, None
    for c in range(1, len(ps)):
        f = int(end[c])
        if f & F.END_NO_MOVES:
            k = (2, 0) if f & F.END_CHECK else (1, 0)
        else:
            s = int(ps[c]) + int(po[c])
            k = (1, -(abs(s) // 16 * (1 if s >= 0 else -1)))  # C truncation
        if key is None or k > key:  # the first maximum
            best, key = c, k
    if not best:
        return (0, 0, 0, len(ps) - 1, 0, 0, F.BEST_NONE, int(end[0]))
    kind = F.BEST_MATE if key[0] == 2 else F.BEST_CP
    return (wrap_neg(ps[best]), wrap_neg(po[best]), key[1] if kind == F.BEST_CP else 0, len(ps) - 1, best,
            int(moves[best]) if moves is not None else 0, kind, int(end[0]))


BEST = dict(zip(("psqt", "positional", "value", "nodes", "best", "move", "kind", "end"), range(8)))


def reply_rule(end, moves, child_best):
    """fnnue_best_replies for one group: end / moves of its records (record 0 = the ply), child_best[c - 1]
    the depth-1 tuple of child c (a child without a legal move: its own terms in psqt / positional).
    -> (psqt, positional, value, nodes, best, reply_index, move, reply, kind, end, pv_len, 0)."""
    n = len(end)
    if n == 0:
        return (0,) * 12
    best, key = 0, None
    for c in range(1, n):
        f, b = int(end[c]), child_best[c - 1]
        if f & F.END_NO_MOVES:
            k = (3, 0) if f & F.END_CHECK else (2, 0)
        elif b[BEST["kind"]] == F.BEST_MATE:
            k = (1, 0)
        else:
            k = (2, -b[BEST["value"]])
        if key is None or k > key:  # higher rank, then higher value, then the lower index
            best, key = c, k
    nodes = n - 1 + sum(b[BEST["nodes"]] for b in child_best[:n - 1])
    if not best:
        return (0, 0, 0, nodes, 0, 0, 0, 0, F.BEST_NONE, int(end[0]), 0, 0)
    b = child_best[best - 1]
    mv = int(moves[best]) if moves is not None else 0
    if int(end[best]) & F.END_NO_MOVES:  # a one-move pv: the child's own terms, negated
        kind = F.BEST_MATE if key[0] == 3 else F.BEST_CP
        return (wrap_neg(b[0]), wrap_neg(b[1]), 0, nodes, best, 0, mv, 0, kind, int(end[0]), 1, 0)
    kind = F.BEST_MATED if key[0] == 1 else F.BEST_CP
    return (b[0], b[1], key[1] if kind == F.BEST_CP else 0, nodes, best, b[BEST["best"]], mv, b[BEST["move"]], kind,
            int(end[0]), 2, 0)


# ---- the reference: host replays, the oracle's terms, the rule ----

def squares(rec):
    """The 64 piece nibbles of a packed record (0 empty, colour << 3 | type 1..6)."""
    b = np.asarray(rec[:32])
    return np.stack([b & 15, b >> 4], axis=1).reshape(64)


def sq_name(s):
    return "abcdefgh"[s & 7] + "12345678"[s >> 3]


def move_text(fen, prefix, parent, child, white, c960):
    """The UCI text of the move between two records of the host builder, found
    from the squares that changed and checked by replaying it.  Castling is
    spelled as the game's notation does: the king's destination, or the rook's
    square in a game that needs Chess960 notation."""
    a, b = squares(parent), squares(child)
    own = lambda x: x != 0 and (x < 8) == white
    changed = [s for s in range(64) if a[s] != b[s]]
    froms = [s for s in changed if own(a[s])] + [s for s in range(64) if a[s] == (6 if white else 14)]
    found = []
    for f in dict.fromkeys(froms):
        for t in changed:
            if t == f:
                continue
            promos = ["n", "b", "r", "q"] if a[f] & 7 == 1 and (t >> 3) in (0, 7) else [""]
            for p in promos:
                text = sq_name(f) + sq_name(t) + p
                try:
                    last = F.game_positions(fen, prefix + [text])[-1]
                except F.FnnueError:
                    continue
                if np.array_equal(last, child):
                    found.append((text, own(a[t])))  # own(a[t]): the king takes its own rook
    if len(found) > 1:
        found = [x for x in found if x[1] == c960]
    assert len(found) == 1, (fen, prefix, found)
    return found[0][0]


def code_of(text):
    s = lambda x: (ord(x[0]) - 97) | (int(x[1]) - 1) << 3
    return s(text[0:2]) | s(text[2:4]) << 6 | (" pnbrq".index(text[4]) if len(text) > 4 else 0) << 12


def expand(fen, prefix, c960):
    """The last ply of (fen, prefix): its records (ply + children), the children's texts, all end flags."""
    hp, ho = F.game_children(fen, prefix)
    grp = hp[int(ho[-2]):int(ho[-1])]
    white = (fen.split()[1] == "w") == (len(prefix) % 2 == 0)
    texts = [move_text(fen, prefix, grp[0], grp[c], white, c960) for c in range(1, len(grp))]
    end = [F.game_end(fen, prefix)] + [F.game_end(fen, prefix + [t]) for t in texts]
    return grp, texts, end


def build_reference(data, games=None):
    """-> (one reply_rule tuple per ply in game order, CHAIN offsets per game,
    per ply the list of its children's (move text, depth-1 tuple or None when the child has no legal move))."""
    games = GAMES if games is None else games
    plies, records = [], []
    for fen, mv in games:
        ms = mv.split()
        c960 = fen == CHESS960
        for q in range(len(ms) + 1):
            grp, texts, end = expand(fen, ms[:q], c960)
            kids = []
            for t in texts:
                g, gt, ge = expand(fen, ms[:q] + [t], c960)
                kids.append((len(records), len(g), gt, ge))
                records.extend(g)
            plies.append((texts, end, kids))
    ps, po, rc = OracleNet(data).eval_packed(np.array(records, dtype=np.uint8).reshape(-1, 36), threads=8)
    assert rc == 0
    out, per_child = [], []
    for texts, end, kids in plies:
        cb, shown = [], []
        for t, (o, n, gt, ge) in zip(texts, kids):
            if n == 1:  # no legal move: its own terms
                cb.append((int(ps[o]), int(po[o]), 0, 0, 0, 0, F.BEST_NONE, ge[0]))
                shown.append((t, None))
            else:
                d1 = reduce_group(ps[o:o + n], po[o:o + n], ge, [0] + [code_of(x) for x in gt])
                cb.append(d1)
                shown.append((t, d1))
        out.append(reply_rule(end, [0] + [code_of(t) for t in texts], cb))
        per_child.append(shown)
    off = np.cumsum([0] + [len(m.split()) + 1 for _, m in games]).astype(np.uint32)
    return out, off, per_child


_REF = {}


def reference():
    """The reference of GAMES on the HD-256 synthetic net: computed once, shared."""
    if "r" not in _REF:
        _REF["r"] = build_reference(net_bytes(1, 256, 0))
    return _REF["r"]


B2 = dict(zip(F.BEST2_DTYPE.names, range(12)))


# ---- the tests ----

def test_best2_record_layout():
    assert F.BEST2_DTYPE.itemsize == 32 and N.BEST2_BYTES == 32
    assert [(n, F.BEST2_DTYPE.fields[n][1]) for n in F.BEST2_DTYPE.names] == \
        [("psqt", 0), ("positional", 4), ("value", 8), ("nodes", 12), ("best", 16), ("reply_index", 20), ("move", 24),
         ("reply", 26), ("kind", 28), ("end", 29), ("pv_len", 30), ("reserved", 31)]
    assert F.BEST_MATED == 4 and N.BEST_MATED == 4
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 7


def test_new_entry_points_refuse_null_arguments():
    n, g, k = C.c_size_t(), C.c_size_t(), C.c_size_t()
    L = N.lib
    assert L.fnnue_backend_set_analysis_plies(None, 2) == E_ARG
    assert L.fnnue_backend_set_analysis_plies(None, 0) == E_ARG
    assert L.fnnue_best_replies_device(None, None, None, None, 1, 1, None, None, None) == E_ARG
    assert L.fnnue_best_replies(None, None, None, None, 1, 1, None, None) == E_ARG
    assert L.fnnue_search2_device(None, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g), None) == E_ARG
    assert L.fnnue_search2(None, b"x", 1, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_search2_children(None, b"x", 1, None, None, 1, None, 0, None, 0, None, None, 0, C.byref(n),
                                    C.byref(g), C.byref(k)) == E_ARG
    assert L.fnnue_backend_go_pv(None, None, 0, None, 0, None, None, None, 0) == E_ARG
    assert L.fnnue_backend_analysis_json_pv(None, 1, None, None, 0, None) == E_ARG
    assert b"null" in L.fnnue_last_error()


def resp(pid, kind, value, depth, nodes, move=None, reply=None, matrix=False, nps=0):
    r = B.PositionResponse(pid, B.Score(kind, value), 1, 2, depth, nodes, 7, nps, move, matrix=matrix)
    r.reply = reply
    return r


def test_json_with_and_without_reply():
    assert B.PositionResponse(0, B.Score("cp", 1)).reply is None
    assert B.into_analysis([resp(0, "cp", -25, 2, 420, "e2e4", "e7e5", nps=1000)]) == \
        '[{"pv":"e2e4 e7e5","score":{"cp":-25},"depth":2,"nodes":420,"time":7,"nps":1000}]'
    assert B.into_analysis([resp(0, "mate", -1, 2, 5, "h1g1", "a2a1"), resp(1, "cp", 3, 2, 9, "a7a8q", "b7a8n")]) == \
        '[{"pv":"h1g1 a2a1","score":{"mate":-1},"depth":2,"nodes":5,"time":7},' \
        '{"pv":"a7a8q b7a8n","score":{"cp":3},"depth":2,"nodes":9,"time":7}]'
    assert B.into_analysis([resp(0, "cp", 31, 2, 20, "e2e4", "e7e5", matrix=True)]) == \
        '[{"pv":[[null,null,["e2e4","e7e5"]]],"score":[[null,null,{"cp":31}]],"depth":2,"nodes":20,"time":7}]'
    # without a reply: byte for byte what it was
    rows = [resp(3, "mate", 1, 1, 31, "d8h4"), resp(4, "mate", 0, 0, 0), B.PositionResponse(5, None, skipped=True),
            resp(6, "cp", 4, 1, 3, "a7a8q", matrix=True)]
    plain = '[{"pv":"d8h4","score":{"mate":1},"depth":1,"nodes":31,"time":7},' \
            '{"score":{"mate":0},"depth":0,"nodes":0,"time":7},{"skipped":true},' \
            '{"pv":[[null,["a7a8q"]]],"score":[[null,{"cp":4}]],"depth":1,"nodes":3,"time":7}]'
    assert B.into_analysis(rows) == plain
    mixed = rows + [resp(7, "cp", 1, 2, 2, "a2a3", "a7a6")]
    assert B.into_analysis(mixed) == plain[:-1] + ',{"pv":"a2a3 a7a6","score":{"cp":1},"depth":2,"nodes":2,"time":7}]'


def test_move_text_finder():
    grp, texts, end = expand(START, [], False)
    assert len(texts) == 20 and set(texts) >= {"e2e4", "g1f3", "a2a3"} and end == [0] * 21
    ms = C960_MOVES.split()
    _, texts, _ = expand(CHESS960, ms[:6], True)
    assert "g1h1" in texts and len(set(texts)) == len(texts)  # the king takes its rook
    _, texts, _ = expand("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", [], False)
    assert "e1g1" in texts and "e1c1" in texts and "e1h1" not in texts
    _, texts, _ = expand("8/P6k/8/8/8/8/6Kp/8 w - - 0 1", [], False)
    assert {"a7a8q", "a7a8n", "a7a8r", "a7a8b"} <= set(texts)
    assert code_of("e7e8q") == 52 | 60 << 6 | 5 << 12 and F.move_uci(code_of("g1h1")) == "g1h1"


def test_reference_covers_every_kind_and_pv_length():
    ref, off, per_child = reference()
    assert off.tolist() == [0, 10, 20, 28, 29, 30, 34, 37, 38, 43] and len(ref) == 43
    assert {r[B2["kind"]] for r in ref} == {F.BEST_NONE, F.BEST_CP, F.BEST_MATE, F.BEST_MATED}
    assert {r[B2["pv_len"]] for r in ref} == {0, 1, 2}
    assert 20000 < sum(r[B2["nodes"]] for r in ref) < 40000
    rec = lambda i: dict(zip(F.BEST2_DTYPE.names, ref[i]))
    # a mate in one is there: a one-move pv
    r = rec(off[I_MATE1] + 3)
    assert (r["kind"], F.move_uci(r["move"]), r["pv_len"], r["reply"], r["value"]) == (F.BEST_MATE, "d8h4", 1, 0, 0)
    # one move earlier g2g4 allows it: that child is never the best while another is there
    r = rec(off[I_BLUNDER] + 2)
    texts = [t for t, _ in per_child[off[I_BLUNDER] + 2]]
    g4 = dict(per_child[off[I_BLUNDER] + 2])["g2g4"]
    assert g4[BEST["kind"]] == F.BEST_MATE and F.move_uci(g4[BEST["move"]]) == "d8h4"
    assert r["kind"] == F.BEST_CP and r["pv_len"] == 2 and texts[r["best"] - 1] != "g2g4"
    assert sum(1 for _, d in per_child[off[I_BLUNDER] + 2] if d[BEST["kind"]] == F.BEST_MATE) == 1
    # every move allows a mate in one: the first child
    r = rec(off[I_MATED])
    assert (r["kind"], r["best"], r["pv_len"], F.move_uci(r["reply"]), r["value"]) == (F.BEST_MATED, 1, 2, "a2a1", 0)
    assert r["nodes"] == 2 + sum(d[BEST["nodes"]] for _, d in per_child[off[I_MATED]])
    # mating and stalemating moves together: the first mate, a one-move pv
    r = rec(off[I_MOS])
    assert r["kind"] == F.BEST_MATE and F.move_uci(r["move"]) in ("f7g7", "f7f8") and r["pv_len"] == 1
    assert any(d is None for _, d in per_child[off[I_MOS]])
    # 218 children
    r = rec(off[I_MANY])
    assert len(per_child[off[I_MANY]]) == 218 and r["nodes"] > 218 and r["kind"] in (F.BEST_MATE, F.BEST_CP)
    # the finished game's last ply
    assert ref[-1] == (0, 0, 0, 0, 0, 0, 0, 0, F.BEST_NONE, F.END_NO_MOVES | F.END_CHECK, 0, 0)
    # the Chess960 game's ply before castling has the castling child
    assert "g1h1" in [t for t, _ in per_child[off[I_C960] + 6]]

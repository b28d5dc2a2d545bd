"""The host side of MultiPV at two plies (ABI 3.11): the layouts of fnnue_line2
and fnnue_pv_line2, the no-device error paths of the new entry points, the
`analysis` JSON with one whole pv per line, and the total order of
include/fnnue.h restated in Python, which the GPU tests
(tests/test_gpu_multipv2.py) hold fnnue_topk_replies, fnnue_vtopk_replies and
the searches' lines to.  The order's first element is pinned here against the
already-pinned rules of the second reduction (reply_rule, vreply_rule)."""
import ctypes as C
import json
import random

import numpy as np

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from tests import test_search2 as R
from tests import test_vsearch2 as V

E_ARG, E_CAPACITY = -1, -10
BEST = R.BEST
L2 = dict(zip(F.LINE2_DTYPE.names, range(10)))
# the fields a ply's fnnue_best2 shares with slot 0 of its lines: (fnnue_best2 name, fnnue_line2 name)
SHARED = [("psqt", "psqt"), ("positional", "positional"), ("value", "value"), ("best", "child"),
          ("reply_index", "reply_index"), ("move", "move"), ("reply", "reply"), ("kind", "kind"), ("pv_len", "pv_len")]


# ---- the total order, in Python ----

def chess_key(f, b):
    """(rank, value) of a child with end byte f and depth-1 tuple b: fnnue.h's ABI 3.7 table."""
    if f & F.END_NO_MOVES:
        return (3, 0) if f & F.END_CHECK else (2, 0)
    if b[BEST["kind"]] == F.BEST_MATE:
        return (1, 0)
    return (2, -b[BEST["value"]])


CHESS_KIND = {3: F.BEST_MATE, 2: F.BEST_CP, 1: F.BEST_MATED}


def ordered_lines(end, moves, child_best, variant):
    """Every child of one group (record 0 = the ply) as a fnnue_line2 tuple, best first: the higher rank, then
    the higher value, then the lower index.
    -> [(psqt, positional, value, child, reply_index, move, reply, kind, pv_len, 0)]."""
    key_of, kinds = (V.child_key, V.KIND) if variant else (chess_key, CHESS_KIND)
    ends_pv = (F.END_WON | F.END_NO_MOVES) if variant else F.END_NO_MOVES
    keyed = [(key_of(int(end[c]), child_best[c - 1]), c) for c in range(1, len(end))]
    keyed.sort(key=lambda kc: (-kc[0][0], -kc[0][1], kc[1]))
    out = []
    for (rank, value), c in keyed:
        b = child_best[c - 1]
        mv = int(moves[c]) if moves is not None else 0
        kind = kinds[rank]
        if int(end[c]) & ends_pv:  # a one-move pv: the child's own terms, negated
            out.append((R.wrap_neg(b[0]), R.wrap_neg(b[1]), 0, c, 0, mv, 0, kind, 1, 0))
        else:
            out.append((b[0], b[1], value if kind == F.BEST_CP else 0, c, b[BEST["best"]], mv, b[BEST["move"]], kind,
                        2, 0))
    return out


def lines_over_groups(end, moves, off, cbt, line_off, variant, cap=None, fill=0):
    """fnnue_[v]topk_replies as the kernel reads its arrays: offsets clamped to len(end), the children's tuples
    dense in record order, group g's slots [line_off[g], line_off[g + 1]) cut at `cap`; a slot beyond the
    children is all-zero, a slot nobody writes keeps the `fill` bytes.  -> a LINE2_DTYPE array of `cap` slots."""
    cap = int(line_off[-1]) if cap is None else cap
    out = np.full(max(cap, 1) * N.LINE2_BYTES, fill, dtype=np.uint8).view(F.LINE2_DTYPE)[:cap]
    base, npos = 0, len(end)
    for g, (o, e) in enumerate(zip(off[:-1], off[1:])):
        e = min(int(e), npos)
        o = min(int(o), e)
        nk = max(e - o - 1, 0)
        if e > o:
            lines = ordered_lines(end[o:e], moves[o:e] if moves is not None else None, cbt[base:base + nk], variant)
            for j in range(int(line_off[g]), min(int(line_off[g + 1]), cap)):
                q = j - int(line_off[g])
                out[j] = lines[q] if q < nk else (0,) * 10
        base += nk
    assert base == len(cbt)
    return out


def shared_of_best2(rec):
    """The fields of a fnnue_best2 tuple that slot 0 repeats, in fnnue_line2 order (reserved left out)."""
    return tuple(rec[R.B2[a]] for a, _ in SHARED)


def shared_of_line(line):
    return tuple(line[L2[b]] for _, b in SHARED)


# ---- layouts and versions ----

def test_line2_record_layout():
    assert F.LINE2_DTYPE.itemsize == 28 and N.LINE2_BYTES == 28
    assert [(n, F.LINE2_DTYPE.fields[n][1]) for n in F.LINE2_DTYPE.names] == \
        [("psqt", 0), ("positional", 4), ("value", 8), ("child", 12), ("reply_index", 16), ("move", 20), ("reply", 22),
         ("kind", 24), ("pv_len", 25), ("reserved", 26)]


def test_pv_line2_record_layout():
    P = B._PvLine2
    assert C.sizeof(P) == 32 and N.PV_LINE2_BYTES == 32
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == \
        [("score", 0), ("psqt", 8), ("positional", 12), ("pv", 16), ("score_kind", 30), ("pv_len", 31)]
    assert P.pv.size == 14


def test_abi_version():
    v = N.lib.fnnue_abi_version()
    assert v >> 16 == 3 and v & 0xFFFF >= 11


# ---- the error paths that need no device ----

def test_new_entry_points_refuse_null_arguments_and_zero_the_counts():
    L, ZH = N.lib, N.VARIANT_CRAZYHOUSE
    for fn in (L.fnnue_topk_replies_device, L.fnnue_vtopk_replies_device):
        assert fn(None, None, None, None, 1, 1, None, None, None, 0, None) == E_ARG
    for fn in (L.fnnue_topk_replies, L.fnnue_vtopk_replies):
        assert fn(None, None, None, None, 1, 1, None, None, None, 0) == E_ARG
    n, g = C.c_size_t(7), C.c_size_t(7)

    def zeroed(rc):
        assert rc == E_ARG and (n.value, g.value) == (0, 0)
        n.value = g.value = 7

    zeroed(L.fnnue_search2_lines_device(None, None, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                        C.byref(g), None))
    zeroed(L.fnnue_search2_lines(None, b"x", 1, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n), C.byref(g)))
    zeroed(L.fnnue_vsearch2_lines_device(None, ZH, None, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                         C.byref(g), None))
    zeroed(L.fnnue_vsearch2_lines(None, ZH, b"x", 1, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                  C.byref(g)))
    assert b"null" in L.fnnue_last_error()
    # the counts too
    assert L.fnnue_search2_lines(None, b"x", 1, None, None, 1, 3, None, 0, None, 0, None, 0, None, None) == E_ARG
    assert L.fnnue_vsearch2_lines(None, ZH, b"x", 1, None, None, 1, 3, None, 0, None, 0, None, 0, None, None) == E_ARG
    # the actor's entries
    assert L.fnnue_backend_go_lines_pv(None, None, 0, None, 0, None, None, None, 0, None, None, 0) == E_ARG
    assert L.fnnue_backend_analysis_json_lines_pv(None, 1, None, None, None, 0, None) == E_ARG


def test_k_outside_1_to_218_is_refused():
    L, ZH = N.lib, N.VARIANT_CRAZYHOUSE
    for k in (0, 219):
        n, g = C.c_size_t(7), C.c_size_t(7)
        assert L.fnnue_search2_lines(None, b"x", 1, None, None, 1, k, None, 0, None, 0, None, 0, C.byref(n),
                                     C.byref(g)) == E_ARG
        assert b"k must be 1..218" in L.fnnue_last_error() and (n.value, g.value) == (0, 0)
        assert L.fnnue_search2_lines_device(None, None, None, None, 1, k, None, 0, None, 0, None, 0, C.byref(n),
                                            C.byref(g), None) == E_ARG
        assert b"k must be 1..218" in L.fnnue_last_error()
        assert L.fnnue_vsearch2_lines(None, ZH, b"x", 1, None, None, 1, k, None, 0, None, 0, None, 0, C.byref(n),
                                      C.byref(g)) == E_ARG
        assert b"k must be 1..218" in L.fnnue_last_error()
        assert L.fnnue_vsearch2_lines_device(None, ZH, None, None, None, 1, k, None, 0, None, 0, None, 0, C.byref(n),
                                             C.byref(g), None) == E_ARG
        assert b"k must be 1..218" in L.fnnue_last_error()


# ---- the JSON ----

def resp(pid, kind, value, depth, nodes, move=None, reply=None, matrix=True, lines=None):
    r = B.PositionResponse(pid, B.Score(kind, value), 1, 2, depth, nodes, 7, 0, move, matrix=matrix)
    r.reply = reply
    r.lines = lines
    return r


def line(kind, value, *pv):
    return B.PvLine2(B.Score(kind, value), list(pv), 5, -6)


def test_json_two_lines_at_depth_two():
    rows = [resp(0, "cp", 31, 2, 420, "e2e4", "e7e5", lines=[line("cp", 31, "e2e4", "e7e5"),
                                                             line("cp", 28, "d2d4", "d7d5")])]
    assert B.into_analysis(rows) == \
        '[{"pv":[[null,null,["e2e4","e7e5"]],[null,null,["d2d4","d7d5"]]],' \
        '"score":[[null,null,{"cp":31}],[null,null,{"cp":28}]],"depth":2,"nodes":420,"time":7}]'


def test_json_a_mate_in_one_above_a_two_move_line_and_a_drop():
    # line 0 mates in one: the response is at depth 1, and every row has one null whatever its own pv's length
    rows = [resp(3, "mate", 1, 1, 50, "d8h4", lines=[line("mate", 1, "d8h4"), line("cp", -9, "a7a6", "g4g5"),
                                                     line("mate", -1, "N@f3", "e7e5")]),
            B.PositionResponse(4, None, skipped=True)]
    text = B.into_analysis(rows)
    assert text == '[{"pv":[[null,["d8h4"]],[null,["a7a6","g4g5"]],[null,["N@f3","e7e5"]]],' \
                   '"score":[[null,{"mate":1}],[null,{"cp":-9}],[null,{"mate":-1}]],"depth":1,"nodes":50,"time":7},' \
                   '{"skipped":true}]'
    parts = json.loads(text)
    assert parts[0]["pv"][2][1] == ["N@f3", "e7e5"] and parts[0]["score"][0][1] == {"mate": 1}


def json_lines_pv(rows, cap=None):
    """fnnue_backend_analysis_json_lines_pv called directly -> (rc, text, needed length)."""
    arr = (B._Response * max(1, len(rows)))()
    for i, r in enumerate(rows):
        if r.skipped:
            arr[i] = B._Response(r.position_id, 1)
            continue
        arr[i] = B._Response(r.position_id, 0, B.SCORE_MATE if r.score.kind == "mate" else B.SCORE_CP, r.depth,
                             1 if r.matrix else 0, r.score.value, r.psqt, r.positional, r.nodes, r.time_ms, r.nps,
                             (r.best_move or "").encode())
    loff = np.zeros(len(rows) + 1, dtype=np.uint32)
    loff[1:] = np.cumsum([len(r.lines or ()) for r in rows])
    pv = (B._PvLine2 * max(1, int(loff[-1])))()
    at = 0
    for r in rows:
        for l in r.lines or ():
            pv[at] = B._PvLine2(l.score.value, l.psqt, l.positional, " ".join(l.pv).encode(),
                                B.SCORE_MATE if l.score.kind == "mate" else B.SCORE_CP, len(l.pv))
            at += 1
    n = C.c_size_t()
    N.lib.fnnue_backend_analysis_json_lines_pv(arr, len(rows), pv, N.ptr(loff), None, 0, C.byref(n))
    size = n.value + 1 if cap is None else cap
    buf = C.create_string_buffer(max(size, 1))
    rc = N.lib.fnnue_backend_analysis_json_lines_pv(arr, len(rows), pv, N.ptr(loff), buf, size, C.byref(n))
    return rc, buf.value.decode(), n.value


def test_json_without_lines_and_with_one_line_equals_json_pv():
    # no lines: fnnue_backend_analysis_json_pv's bytes for the same rows (which have no reply)
    plain = [resp(0, "cp", 4, 1, 3, "a7a8q"), resp(1, "mate", 0, 0, 0), B.PositionResponse(2, None, skipped=True),
             resp(3, "cp", -25, 1, 20, "e2e4", matrix=False)]
    rc, text, _ = json_lines_pv(plain)
    assert rc == 0 and text == B.into_analysis(plain)
    # one line each: the two-move pv fnnue_backend_analysis_json_pv prints from the reply
    one = [resp(0, "cp", 31, 2, 20, "e2e4", "e7e5", lines=[line("cp", 31, "e2e4", "e7e5")]),
           resp(1, "mate", 1, 1, 9, "d8h4", lines=[line("mate", 1, "d8h4")]),
           resp(2, "mate", -1, 2, 9, "R@e8", "Q@f2", lines=[line("mate", -1, "R@e8", "Q@f2")])]
    rc, text, _ = json_lines_pv(one)
    with_reply = [resp(r.position_id, r.score.kind, r.score.value, r.depth, r.nodes, r.best_move, r.reply)
                  for r in one]
    assert rc == 0 and text == B.into_analysis(with_reply) == B.into_analysis(one)
    assert '"pv":[[null,null,["e2e4","e7e5"]]]' in text
    # lines are rows of the matrix form only
    best = [resp(0, "cp", 31, 2, 20, "e2e4", matrix=False, lines=[line("cp", 31, "e2e4", "e7e5"),
                                                                  line("cp", 3, "d2d4", "d7d5")])]
    rc, text, _ = json_lines_pv(best)
    assert rc == 0 and text == '[{"pv":"e2e4","score":{"cp":31},"depth":2,"nodes":20,"time":7}]'


def test_json_buffer_too_small():
    rows = [resp(0, "cp", 31, 2, 420, "e2e4", "e7e5", lines=[line("cp", 31, "e2e4", "e7e5"),
                                                             line("cp", 28, "d2d4", "d7d5")])]
    rc, full, need = json_lines_pv(rows)
    assert rc == 0 and need == len(full)
    rc, text, n = json_lines_pv(rows, cap=need)  # no room for the NUL
    assert rc == E_CAPACITY and text == "" and n == need
    rc, text, n = json_lines_pv(rows, cap=need + 1)
    assert rc == 0 and text == full


# ---- the order against the pinned rules ----

def random_group(rnd, variant):
    n = rnd.randrange(0, 14)
    if variant:
        flags = [0, 0, 0, F.END_CHECK, F.END_NO_MOVES, F.END_NO_MOVES | F.END_CHECK, F.END_NO_MOVES | F.END_EXTINCT,
                 F.END_NO_MOVES | F.END_VARIANT, F.END_WON, F.END_WON | F.END_NO_MOVES | F.END_VARIANT]
        kinds = (F.BEST_NONE, F.BEST_CP, F.BEST_CP, F.BEST_CP, F.BEST_MATE, F.BEST_LOST)
    else:
        flags = [0, 0, 0, 1, 2, 3]
        kinds = (F.BEST_NONE, F.BEST_CP, F.BEST_CP, F.BEST_MATE)
    end = [rnd.choice(flags) for _ in range(n)]
    cb = [V.kid(rnd.choice(kinds), rnd.randrange(-6, 6), rnd.randrange(9), rnd.randrange(1, 9),
                rnd.randrange(1, 4096), rnd.randrange(-99, 99), rnd.randrange(-99, 99)) for _ in range(max(n - 1, 0))]
    return end, list(range(100, 100 + n)), cb


def test_first_line_equals_the_reduction_rules_on_random_groups():
    rnd = random.Random(11)
    seen = set()
    for variant, rule in ((False, R.reply_rule), (True, V.vreply_rule)):
        for _ in range(600):
            end, moves, cb = random_group(rnd, variant)
            lines = ordered_lines(end, moves, cb, variant)
            assert len(lines) == max(len(end) - 1, 0)
            assert sorted(l[L2["child"]] for l in lines) == list(range(1, len(end)))
            best2 = rule(end, moves, cb)
            if lines:
                assert shared_of_line(lines[0]) == shared_of_best2(best2), (end, cb)
            else:
                assert best2[R.B2["kind"]] == F.BEST_NONE
            seen |= {(variant, l[L2["kind"]], l[L2["pv_len"]]) for l in lines}
            without = ordered_lines(end, None, cb, variant)
            assert [l[:5] + (0,) + l[6:] for l in lines] == without
    assert {(False, F.BEST_MATE, 1), (False, F.BEST_CP, 1), (False, F.BEST_CP, 2), (False, F.BEST_MATED, 2),
            (True, F.BEST_LOST, 1), (True, F.BEST_MATE, 1), (True, F.BEST_MATE, 2), (True, F.BEST_MATED, 2),
            (True, F.BEST_CP, 1), (True, F.BEST_CP, 2)} <= seen


def test_order_classes_and_ties():
    kid = V.kid
    # chess: two mates in index order, values descending with the stalemating move at 0, ties by index, mated last
    end = [0, 0, 3, 0, 1, 3, 0, 0]
    cb = [kid(F.BEST_MATE), kid(F.BEST_NONE), kid(value=-5), kid(F.BEST_NONE, ps=4), kid(F.BEST_NONE), kid(value=0),
          kid(value=-5)]
    lines = ordered_lines(end, None, cb, False)
    assert [l[L2["child"]] for l in lines] == [2, 5, 3, 7, 4, 6, 1]
    assert [l[L2["kind"]] for l in lines] == [F.BEST_MATE] * 2 + [F.BEST_CP] * 4 + [F.BEST_MATED]
    assert [l[L2["value"]] for l in lines] == [0, 0, 5, 5, 0, 0, 0] and lines[4][L2["psqt"]] == -4
    # variants: mate in one, every reply loses, values, the reply wins, lost; each class in index order
    W = F.END_WON
    end = [0, W, 0, 0, 0, F.END_NO_MOVES | F.END_VARIANT, 0, W | F.END_NO_MOVES, 0, F.END_NO_MOVES]
    cb = [kid(), kid(F.BEST_MATE), kid(value=3), kid(F.BEST_LOST, best=2, move=9), kid(F.BEST_NONE), kid(F.BEST_LOST),
          kid(F.BEST_NONE), kid(F.BEST_MATE), kid(F.BEST_NONE)]
    lines = ordered_lines(end, None, cb, True)
    assert [l[L2["child"]] for l in lines] == [5, 4, 6, 9, 3, 2, 8, 1, 7]
    assert [l[L2["kind"]] for l in lines] == [F.BEST_MATE] * 3 + [F.BEST_CP] * 2 + [F.BEST_MATED] * 2 + [F.BEST_LOST] * 2
    assert [l[L2["pv_len"]] for l in lines] == [1, 2, 2, 1, 2, 2, 2, 1, 1]
    assert (lines[1][L2["reply_index"]], lines[1][L2["reply"]]) == (2, 9)
    # the slots of several groups: beyond the children all-zero, an empty group and a cut keep the fill
    end = np.array([0, 0, 0, 0, 0], dtype=np.uint8)
    off = [0, 3, 3, 4, 9]  # 2 children, empty, no child, cut by npos to one record
    got = lines_over_groups(end, None, off, [kid(value=1), kid(value=-1)], [0, 3, 5, 6, 8], False, cap=7, fill=0xAB)
    assert [int(x) for x in got["child"][:3]] == [2, 1, 0] and got[2].tobytes() == bytes(28)
    assert got[3:5].tobytes() == b"\xab" * 56 and got[5].tobytes() == bytes(28) and got[6].tobytes() == bytes(28)

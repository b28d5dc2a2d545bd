"""The host side of the variant two-ply search (ABI 3.10): the ABI version,
the no-device error paths of the new entry points and of the new setter, the
`analysis` JSON with a two-move pv that holds a drop, and the rule of
include/fnnue.h restated in Python, which the GPU tests
(tests/test_gpu_vsearch2.py) hold fnnue_vbest_replies and fnnue_vsearch2 to."""
import ctypes as C

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B

E_ARG = -1
WON = F.END_WON
DECIDED = F.END_CHECK | F.END_EXTINCT | F.END_VARIANT
BEST = dict(zip(("psqt", "positional", "value", "nodes", "best", "move", "kind", "end"), range(8)))


# ---- the rule, in Python ----

def wrap_neg(x):
    return ((-int(x) + 2**31) % 2**32) - 2**31


def child_key(f, b):
    """(rank, value) of a child with end byte f and depth-1 tuple b, the conditions in the header's order."""
    if f & WON:
        return (0, 0)
    if f & F.END_NO_MOVES:
        return (4, 0) if f & DECIDED else (2, 0)
    if b[BEST["kind"]] == F.BEST_LOST:
        return (3, 0)
    if b[BEST["kind"]] == F.BEST_MATE:
        return (1, 0)
    return (2, -b[BEST["value"]])


KIND = {0: F.BEST_LOST, 1: F.BEST_MATED, 2: F.BEST_CP, 3: F.BEST_MATE, 4: F.BEST_MATE}


def vreply_rule(end, moves, child_best):
    """fnnue_vbest_replies for one group: end / moves of its records (record 0 = the ply), child_best[c - 1]
    the depth-1 tuple of child c (a child without a legal move: its own terms in psqt / positional).
    -> (psqt, positional, value, nodes, best, reply_index, move, reply, kind, end, pv_len, 0)."""
    n = len(end)
    if n == 0:
        return (0,) * 12
    best, key = 0, None
    for c in range(1, n):
        k = child_key(int(end[c]), child_best[c - 1])
        if key is None or k > key:  # higher rank, then higher value, then the lower index
            best, key = c, k
    nodes = n - 1 + sum(b[BEST["nodes"]] for b in child_best[:n - 1])
    if not best:
        return (0, 0, 0, nodes, 0, 0, 0, 0, F.BEST_NONE, int(end[0]), 0, 0)
    b = child_best[best - 1]
    mv = int(moves[best]) if moves is not None else 0
    kind = KIND[key[0]]
    if int(end[best]) & (WON | F.END_NO_MOVES):  # a one-move pv: the child's own terms, negated
        return (wrap_neg(b[0]), wrap_neg(b[1]), 0, nodes, best, 0, mv, 0, kind, int(end[0]), 1, 0)
    return (b[0], b[1], key[1] if kind == F.BEST_CP else 0, nodes, best, b[BEST["best"]], mv, b[BEST["move"]], kind,
            int(end[0]), 2, 0)


def vrule_over_groups(end, moves, off, cbt):
    """vreply_rule over STAR groups as the kernel reads them: offsets clamped to len(end), the children's
    tuples dense in record order."""
    out, base, npos = [], 0, len(end)
    for o, e in zip(off[:-1], off[1:]):
        e = min(int(e), npos)
        o = min(int(o), e)
        nk = max(e - o - 1, 0)
        out.append(vreply_rule(end[o:e], moves[o:e] if moves is not None else None, cbt[base:base + nk]))
        base += nk
    assert base == len(cbt)
    return out


def kid(kind=F.BEST_CP, value=0, nodes=0, best=1, move=77, ps=0, po=0):
    return (ps, po, value if kind == F.BEST_CP else 0, nodes, best, move, kind, 0)


# ---- the tests ----

def test_abi_minor():
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 10
    assert N.lib.fnnue_abi_version() >> 16 == 3


def test_new_entry_points_refuse_null_arguments_and_zero_the_counts():
    L, V = N.lib, N.VARIANT_CRAZYHOUSE
    assert L.fnnue_vbest_replies_device(None, None, None, None, 1, 1, None, None, None) == E_ARG
    assert L.fnnue_vbest_replies(None, None, None, None, 1, 1, None, None) == E_ARG
    n, g, k = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    assert L.fnnue_vsearch2_device(None, V, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g), None) == E_ARG
    assert (n.value, g.value) == (0, 0)
    n.value = g.value = 7
    assert L.fnnue_vsearch2(None, V, b"x", 1, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert (n.value, g.value) == (0, 0)  # the counts come back zeroed
    n.value = g.value = 7
    assert L.fnnue_vsearch2_children(None, V, b"x", 1, None, None, 1, None, 0, None, 0, None, None, 0, C.byref(n),
                                     C.byref(g), C.byref(k)) == E_ARG
    assert (n.value, g.value, k.value) == (0, 0, 0)
    assert b"null" in L.fnnue_last_error()
    # the counts too
    assert L.fnnue_vsearch2(None, V, b"x", 1, None, None, 1, None, 0, None, 0, None, None) == E_ARG
    assert L.fnnue_vsearch2_children(None, V, b"x", 1, None, None, 1, None, 0, None, 0, None, None, 0, C.byref(n),
                                     C.byref(g), None) == E_ARG


def test_set_variant_analysis_plies_null_backend_and_old_setter():
    for plies in (0, 1, 2, 3):
        assert N.lib.fnnue_backend_set_variant_analysis_plies(None, plies) == E_ARG
    assert N.lib.fnnue_backend_set_variant_analysis_depth(None, 2) == E_ARG


def test_rule_rows_and_their_order():
    # every row of the table, as the only child
    rows = [((WON, kid(value=5, ps=3, po=-4)), (F.BEST_LOST, 1, 0)),
            ((WON | F.END_NO_MOVES | F.END_VARIANT, kid(F.BEST_NONE, ps=3)), (F.BEST_LOST, 1, 0)),
            ((F.END_NO_MOVES | F.END_CHECK, kid(F.BEST_NONE)), (F.BEST_MATE, 1, 0)),
            ((F.END_NO_MOVES | F.END_EXTINCT, kid(F.BEST_NONE)), (F.BEST_MATE, 1, 0)),
            ((F.END_NO_MOVES | F.END_VARIANT, kid(F.BEST_NONE)), (F.BEST_MATE, 1, 0)),
            ((F.END_NO_MOVES, kid(F.BEST_NONE, ps=9)), (F.BEST_CP, 1, 0)),
            ((0, kid(F.BEST_LOST, best=4, move=9)), (F.BEST_MATE, 2, 0)),
            ((0, kid(F.BEST_MATE, best=4, move=9)), (F.BEST_MATED, 2, 0)),
            ((F.END_CHECK, kid(value=-31, best=4, move=9)), (F.BEST_CP, 2, 31))]
    for (f, b), (kind, pv_len, value) in rows:
        r = vreply_rule([0, f], [0, 5], [b])
        assert (r[8], r[10], r[2], r[4]) == (kind, pv_len, value, 1), (f, b)
        assert (r[5], r[7]) == ((b[4], b[5]) if pv_len == 2 else (0, 0))
        assert (r[0], r[1]) == ((b[0], b[1]) if pv_len == 2 else (wrap_neg(b[0]), wrap_neg(b[1])))
    # the ranks: lost < the reply wins < any value < every reply loses < mate in one
    ladder = [(WON, kid()), (0, kid(F.BEST_MATE)), (0, kid(value=2**28)), (0, kid(value=-2**28)), (0, kid(F.BEST_LOST)),
              (F.END_NO_MOVES | F.END_VARIANT, kid(F.BEST_NONE))]
    keys = [child_key(f, b) for f, b in ladder]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for lo in range(len(ladder) - 1):
        for pair in ((lo, lo + 1), (lo + 1, lo)):
            r = vreply_rule([0] + [ladder[i][0] for i in pair], None, [ladder[i][1] for i in pair])
            assert r[4] == pair.index(lo + 1) + 1
    # ties: the lower index; no child: NONE with the ply's own flags; an empty group: zeros
    assert vreply_rule([0, 0, 0], None, [kid(value=3), kid(value=3)])[4] == 1
    assert vreply_rule([9], None, []) == (0, 0, 0, 0, 0, 0, 0, 0, F.BEST_NONE, 9, 0, 0)
    assert vreply_rule([], None, []) == (0,) * 12
    # nodes: the children and theirs, a lost child's included
    assert vreply_rule([0, WON, 0], None, [kid(nodes=4), kid(nodes=6)])[3] == 12


def test_rule_equals_the_chess_rule_on_chess_inputs():
    from tests.test_search2 import reply_rule
    import random
    rnd = random.Random(3)
    for _ in range(300):
        n = rnd.randrange(0, 12)
        end = [rnd.randrange(4) for _ in range(n)]
        cb = [kid(rnd.choice((F.BEST_NONE, F.BEST_CP, F.BEST_CP, F.BEST_MATE)), rnd.randrange(-50, 50), rnd.randrange(9),
                  rnd.randrange(1, 9), rnd.randrange(1, 4096), rnd.randrange(-99, 99), rnd.randrange(-99, 99))
              for _ in range(max(n - 1, 0))]
        moves = list(range(100, 100 + n))
        assert vreply_rule(end, moves, cb) == reply_rule(end, moves, cb)


def resp(pid, kind, value, depth, nodes, move=None, reply=None, matrix=False):
    r = B.PositionResponse(pid, B.Score(kind, value), 1, 2, depth, nodes, 7, 0, move, matrix=matrix)
    r.reply = reply
    return r


def test_json_with_a_two_move_pv_holding_a_drop():
    assert B.into_analysis([resp(0, "cp", -25, 2, 420, "N@f3", "e7e5")]) == \
        '[{"pv":"N@f3 e7e5","score":{"cp":-25},"depth":2,"nodes":420,"time":7}]'
    assert B.into_analysis([resp(0, "mate", -1, 2, 9, "e2e4", "Q@f2"), resp(1, "mate", 1, 2, 5, "a7a8q", "p@h2")]) == \
        '[{"pv":"e2e4 Q@f2","score":{"mate":-1},"depth":2,"nodes":9,"time":7},' \
        '{"pv":"a7a8q P@h2","score":{"mate":1},"depth":2,"nodes":5,"time":7}]'
    assert B.into_analysis([resp(0, "cp", 31, 2, 20, "R@e8", "R@f8", matrix=True)]) == \
        '[{"pv":[[null,null,["R@e8","R@f8"]]],"score":[[null,null,{"cp":31}]],"depth":2,"nodes":20,"time":7}]'
    # chess replies print as they did
    assert B.into_analysis([resp(0, "cp", 3, 2, 9, "a7a8q", "b7a8n")]) == \
        '[{"pv":"a7a8q b7a8n","score":{"cp":3},"depth":2,"nodes":9,"time":7}]'

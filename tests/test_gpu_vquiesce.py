"""The variants' capture quiescence on the device (ABI 3.15), bit-exact and field by field:
fnnue_vquiesce against the rule in Python (tests/test_vquiesce.py vq_ref) for all five
variants, both checks settings and two nets, over every ply of the hand-made positions and
two short games per variant; frontiers of 63 / 64 / 65 expanding nodes; the smallest
budgets; the five variant searches against the existing Python reductions over
reference-substituted leaves; depth 0 byte-identical to a context that never had the
setting, the chess and the variant contexts ignoring each other's setters; and the engine
actor with its mate mapping."""
import json

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import backend as B
from tests import test_multipv2 as M2
from tests import test_vquiesce as V
from tests import test_vsearch2 as R2
from tests.conftest import net_bytes
from tests.test_gpu_multipv2 import slot_offsets
from tests.test_gpu_quiesce import env
from tests.test_gpu_vsearch1 import RK_CATCH, reduce_groups, topk_groups
from tests.test_gpu_vsearch2 import NAME, NORM, as_tuples, bodies_of, strip, trunc_div
from tests.test_vquiesce import AT, KOTH, RK, TC, VARIANTS, ZH

pytestmark = pytest.mark.gpu

K = 3
IDS = [NAME[v] for v in VARIANTS]
SKIP_LEAF = F.END_NO_MOVES | F.END_DRAW | F.END_WON
# the searches' games: few pieces, so that every leaf of two plies can have its reference computed
ZH_FORCED = ("4r2k/6pp/7N/8/8/8/8/K3R3[r] w - - 0 1", "e1e8")   # R@f8 / R@g8, and either is taken with mate
SGAMES = {
    ZH: [(V.ZH_DROP[0], "e1e8 r@f8"), V.ZH_NO_DROP],
    AT: [V.AT_OWN_KING, V.AT_DEFENDED, ("4k3/5p2/8/6N1/8/8/8/4K3 w - - 0 1", "")],
    KOTH: [V.KOTH_HILL, V.AT_DEFENDED, ("8/8/3k4/8/8/3K4/8/8 w - - 0 1", "")],
    RK: [V.RK_GOAL, V.RK_CATCH_UP, RK_CATCH],
    TC: [V.TC_LAST, V.TC_TWO, V.AT_DEFENDED],
}


@pytest.fixture(scope="module")
def evs():
    """Per net kind a crazyhouse and an atomic context (the atomic net serves the three plain variants)."""
    made = {(kind, nv): F.Evaluator(F.Net.from_bytes_variant(V.net_data(nv, kind), nv), 0)
            for kind in ("random", "material") for nv in (ZH, AT)}
    yield made
    for e in made.values():
        e.close()


def serving(evs, v, kind="random"):
    return evs[(kind, V.net_variant(v))]


def with_vquiesce(e, d, checks, fn):
    e.set_search_vquiesce(d, checks)
    try:
        return fn()
    finally:
        e.set_search_vquiesce(0, False)


def results(e, v, games):
    s1, off = e.vsearch1(v, games)
    _, _, l1 = e.vsearch1_lines(v, games, K)
    s2, _, kb, km = e.vsearch2(v, games, children=True)
    s2b, _, l2 = e.vsearch2_lines(v, games, K)
    assert s2b.tobytes() == s2.tobytes()
    return {"off": off, "s1": s1, "l1": l1, "s2": s2, "l2": l2, "kb": kb, "km": km}


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- 1. fnnue_vquiesce against the rule ----

@pytest.mark.parametrize("kind", ["random", "material"])
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_vquiesce_matches_the_rule_field_by_field(evs, v, kind):
    e = serving(evs, v, kind)
    games = V.GAMES[v]
    woff = np.cumsum([0] + [len(mv.split()) + 1 for _, mv in games])
    plies = [(fen, " ".join(mv.split()[:q])) for fen, mv in games for q in range(len(mv.split()) + 1)]
    for d in range(4):
        for checks in (False, True):
            got, off = e.vquiesce(v, games, d, checks)
            want = V.reference(v, kind, d, checks)
            assert off.tolist() == woff.tolist() and len(got) == len(want) == len(plies)   # no ply left out
            for p, (g, w) in enumerate(zip(V.quiet_tuples(got), want)):
                assert g == w, (NAME[v], kind, d, checks, p, plies[p], g, w)


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_depth_four_above_the_trees_height(evs, v):
    e, o = serving(evs, v, "material"), V.oracle_of(v, "material")
    games = V.HAND[v]
    for checks in (False, True):
        got, _ = e.vquiesce(v, games, 4, checks)
        want = [V.vq_ref(o, v, fen, " ".join(mv.split()[:q]), 4, checks)
                for fen, mv in games for q in range(len(mv.split()) + 1)]
        assert V.quiet_tuples(got) == want and max(w[5] for w in want) < 4


def test_the_named_results(evs):
    at, zh = serving(evs, AT, "material"), serving(evs, ZH, "material")
    got, _ = at.vquiesce(AT, [V.AT_NXF7], 1, False)          # Nxf7 explodes the king: decided with checks off
    last = got[-1]
    assert (int(last["value"]), F.vmove_uci(int(last["move"])), int(last["len"]), int(last["reserved"])) == \
        (31999, "g5f7", 1, F.QUIET_DECIDED)
    got, _ = at.vquiesce(AT, [V.AT_DEFENDED], 2, True)       # Qxe5 would lose the queen: stand pat
    assert (int(got[0]["value"]), int(got[0]["len"])) == (700, 0)
    for v, game in ((KOTH, V.KOTH_HILL), (RK, V.RK_GOAL), (TC, V.TC_LAST)):
        got, _ = at.vquiesce(v, [game], 1, False)
        assert (int(got[0]["value"]), int(got[0]["len"]), int(got[0]["reserved"])) == (31999, 1, 1), NAME[v]
    for v, game in ((RK, V.RK_CATCH_UP), (TC, V.TC_TWO)):
        got, _ = at.vquiesce(v, [game], 1, True)
        assert int(got[0]["reserved"]) == 0 and abs(int(got[0]["value"])) < V.DOMAIN, NAME[v]
    on, _ = zh.vquiesce(ZH, [(V.ZH_NO_DROP[0], "")], 1, True)
    off, _ = zh.vquiesce(ZH, [(V.ZH_NO_DROP[0], "")], 1, False)
    assert int(on[0]["value"]) == 31999 and int(off[0]["value"]) == V.VM.vbalance(V.ZH_NO_DROP[0]) + 1000
    got, _ = zh.vquiesce(ZH, [(V.ZH_DROP[0], "e1e8")], 1, True)
    assert F.vmove_uci(int(got[1]["move"])) == "R@f8"        # a line that starts with a drop


def test_arch_and_argument_errors(evs):
    zh, at = serving(evs, ZH), serving(evs, AT)
    chess = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
    try:
        for e, v, code in ((chess, AT, V.E_ARCH), (zh, AT, V.E_ARCH), (at, ZH, V.E_ARCH), (at, 0, V.E_ARCH),
                           (at, 99, V.E_ARCH)):
            with pytest.raises(F.FnnueError) as err:
                e.vquiesce(v, [V.AT_DEFENDED], 1, True)
            assert err.value.code == code
        with pytest.raises(F.FnnueError) as err:
            at.vquiesce(AT, [V.AT_DEFENDED], F.QUIESCE_MAX + 1, True)
        assert err.value.code == V.E_ARG
        with pytest.raises(F.FnnueError) as err:
            at.set_search_vquiesce(F.QUIESCE_MAX + 1)
        assert err.value.code == V.E_ARG
        with pytest.raises(F.FnnueError) as err:
            at.vquiesce(AT, [(V.CHESS_START, "e2e4 e2e4")], 1, True)
        assert err.value.code == V.E_MOVE
        chess.set_search_vquiesce(2, True)               # accepted, and ignored by the chess searches
        assert chess.search_vquiesce() == (2, True)
    finally:
        chess.close()


# ---- 2. frontiers and budgets ----

@pytest.mark.parametrize("n", [63, 64, 65])
@pytest.mark.parametrize("v,game", [(ZH, (V.ZH_DROP[0], "e1e8")), (TC, (V.TC_TWO[0], "h5f7"))],
                         ids=["crazyhouse", "threeCheck"])
def test_a_frontier_of_63_64_65_expanding_nodes(evs, v, game, n):
    e = serving(evs, v)
    one, _ = e.vquiesce(v, [game], 3, True)
    assert int(one["nodes"][0]) >= 1 and int(one["nodes"][1]) >= 2      # both plies expand
    got, _ = e.vquiesce(v, [game] * n, 3, True)
    assert len(got) == 2 * n and got.tobytes() == np.tile(one, n).tobytes()


@pytest.mark.parametrize("v", [ZH, AT, RK], ids=["crazyhouse", "atomic", "racingKings"])
def test_results_do_not_depend_on_the_budgets(evs, v):
    e = serving(evs, v)
    games = V.GAMES[v] * 6                                   # more roots than the smallest budget holds
    want = e.vquiesce(v, games, 3, True)[0]
    assert len(want) > 256
    wres = with_vquiesce(e, 2, True, lambda: results(e, v, SGAMES[v]))
    with env(FNNUE_QUIESCE_RECORDS=256, FNNUE_SEARCH2_RECORDS=1):
        before = e.quiesce_slices()
        got = e.vquiesce(v, games, 3, True)[0]
        assert e.quiesce_slices() - before > 1
        gres = with_vquiesce(e, 2, True, lambda: results(e, v, SGAMES[v]))
    assert got.tobytes() == want.tobytes() and same(gres, wres)


# ---- 3. the five searches against the Python rules over reference-substituted leaves ----

def searches_reference(e, v, games, d, checks):
    """The one-ply and two-ply results of `games` by the existing Python rules, every participating leaf's terms
    replaced by those of vq_ref.  The groups' records, move codes and end flags are the device builder's (held
    to the host elsewhere); the terms are the oracle's."""
    o = V.oracle_of(v, "random")

    def terms(pos):
        ps, po, rc = o.eval_packed(pos)
        assert rc == 0
        return [int(x) for x in ps], [int(x) for x in po]

    counts = {"searched": 0, "skipped": 0, "decided": 0}

    def substitute(ps, po, end, moves, o0, e0, fen, prefix, p):
        for r in range(o0 + 1, e0):
            if int(end[r]) & SKIP_LEAF:
                counts["skipped"] += 1
                continue
            q = V.vq_ref(o, v, fen, (prefix + " " + F.vmove_uci(int(moves[r]))).strip(), d, checks, (ps[r], po[r]))
            ps[r], po[r] = V.leaf_terms(q, p)
            counts["searched"] += 1
            counts["decided"] += q[6]

    pos, coff, moves, end = e.build_vchildren(v, games)
    plies = [(fen, " ".join(mv.split()[:q])) for fen, mv in games for q in range(len(mv.split()) + 1)]
    assert len(plies) == len(coff) - 1
    ps, po = terms(pos)
    for p, (fen, prefix) in enumerate(plies):
        substitute(ps, po, end, moves, int(coff[p]), int(coff[p + 1]), fen, prefix, 1)
    one = reduce_groups(ps, po, end, moves, coff)
    lines1 = topk_groups(ps, po, end, moves, coff, K)
    # two plies: every child's own group, its grandchildren substituted at p = 2
    ext = [(fen, (prefix + " " + F.vmove_uci(int(moves[r]))).strip())
           for p, (fen, prefix) in enumerate(plies) for r in range(int(coff[p]) + 1, int(coff[p + 1]))]
    kb = []
    if ext:
        xpos, xoff, xmoves, xend = e.build_vchildren(v, ext)
        xps, xpo = terms(xpos)
        last = np.cumsum([len(mv.split()) + 1 for _, mv in ext]) - 1     # each extended game's last ply
        for (fen, mv), g in zip(ext, last):
            o0, e0 = int(xoff[g]), int(xoff[g + 1])
            if e0 - o0 == 1:   # no legal move: its own terms
                kb.append((xps[o0], xpo[o0], 0, 0, 0, 0, F.BEST_NONE, int(xend[o0])))
                continue
            substitute(xps, xpo, xend, xmoves, o0, e0, fen, mv, 2)
            kb.append(reduce_groups(xps[o0:e0], xpo[o0:e0], xend[o0:e0], xmoves[o0:e0], [0, e0 - o0])[0])
    two = R2.vrule_over_groups(end, moves, coff, kb)
    lines2 = M2.lines_over_groups(end, moves, coff, kb, slot_offsets([K] * len(plies)), True)
    return {"one": one, "lines1": lines1, "kb": kb, "two": two, "lines2": lines2, "counts": counts}


@pytest.mark.parametrize("checks", [False, True], ids=["plain", "checks"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_searches_match_the_rules_over_substituted_leaves(evs, v, d, checks):
    e = serving(evs, v)
    games = SGAMES[v]
    ref = searches_reference(e, v, games, d, checks)
    got = with_vquiesce(e, d, checks, lambda: results(e, v, games))
    s1, s2 = as_tuples(got["s1"]), as_tuples(got["s2"])
    assert len(s1) == len(s2) == len(ref["one"])
    for p in range(len(s1)):
        assert s1[p] == ref["one"][p], (p, s1[p], ref["one"][p])
        assert s2[p] == ref["two"][p], (p, s2[p], ref["two"][p])
        assert as_tuples(got["l1"][p]) == ref["lines1"][p], p
    kbt = as_tuples(got["kb"])
    assert len(kbt) == len(ref["kb"])
    for k, (a, b) in enumerate(zip(kbt, ref["kb"])):
        assert a == b, (k, a, b)
    assert got["l2"].reshape(-1).tobytes() == ref["lines2"].tobytes()
    c = ref["counts"]
    # untouched leaves and coded mates occur (crazyhouse has no end of its own: its decided leaves are mates)
    assert c["searched"] > 20 and c["skipped"] >= 1 and (c["decided"] >= 1 or (v == ZH and not checks)), c
    plain = results(e, v, games)
    assert not same(plain, got)                                               # the setting does reach the leaves


# ---- 4. depth 0, and the contexts that ignore a setter ----

def test_depth_zero_and_foreign_setters_change_no_byte(evs):
    for v in (ZH, TC):
        e = serving(evs, v)
        fresh = F.Evaluator(F.Net.from_bytes_variant(V.net_data(v, "random"), V.net_variant(v)), 0)
        try:
            want = results(fresh, v, SGAMES[v])
            assert same(results(e, v, SGAMES[v]), want)                       # used with the setting before, now off
            assert same(with_vquiesce(e, 0, True, lambda: results(e, v, SGAMES[v])), want)   # depth 0, checks on
            fresh.set_search_quiesce(2)                                       # the chess setters: still ignored
            fresh.set_search_quiesce_checks(True)
            assert same(results(fresh, v, SGAMES[v]), want)
        finally:
            fresh.close()
    from tests.test_gpu_quiesce import results as chess_results, same as chess_same
    from tests.test_gpu_quiesce_checks import SGAMES as CHESS_GAMES
    a = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
    b = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
    try:
        b.set_search_vquiesce(2, True)
        a.set_search_quiesce(1)
        b.set_search_quiesce(1)
        assert chess_same(chess_results(a, CHESS_GAMES), chess_results(b, CHESS_GAMES))
        assert a.quiesce(CHESS_GAMES, 2)[0].tobytes() == b.quiesce(CHESS_GAMES, 2)[0].tobytes()
    finally:
        a.close()
        b.close()


# ---- 5. the actor ----

def want_score(kind, value):
    if kind == F.BEST_MATE:
        return B.Score("mate", 1)
    if kind in (F.BEST_MATED, F.BEST_LOST):
        return B.Score("mate", -1)
    if abs(value) > V.DOMAIN:
        plies = V.MATE - abs(value)
        return B.Score("mate", (plies + 1) // 2 if value > 0 else -(plies // 2))
    return B.Score("cp", trunc_div(value * 100, NORM))


def make_channel(**kw):
    chess = F.Net.from_bytes(net_bytes(1, 256, 0))
    return B.channel(chess, 0, crazyhouse=F.Net.from_bytes_variant(V.net_data(ZH, "random"), ZH),
                     atomic=F.Net.from_bytes_variant(V.net_data(AT, "random"), AT), **kw)


def test_actor_matches_the_library_and_answers_mates(evs):
    made = [make_channel(variant_analysis_depth=1, variant_quiesce=1, variant_quiesce_checks=True),
            make_channel(variant_analysis_plies=2, variant_quiesce=1, variant_quiesce_checks=True),
            make_channel(variant_analysis_depth=1), make_channel()]
    try:
        c1, c2, p1, d0 = (stub for stub, _ in made)
        assert c1.variant_quiesce() == (1, True) and p1.variant_quiesce() == (0, False)
        mates = 0
        for v in (ZH, AT):
            e = serving(evs, v)
            games = SGAMES[v] + V.GAMES[v][:1]
            bodies = bodies_of(v, games)
            best, goff = with_vquiesce(e, 1, True, lambda: e.vsearch1(v, games))
            out, off = with_vquiesce(e, 1, True, lambda: e.vsearch2(v, games))[:2]
            for res, recs, roff, two in ((c1.go(bodies), best, goff, False), (c2.go_pv(bodies), out, off, True)):
                for i, rows in enumerate(res):
                    assert not isinstance(rows, B.PositionFailed), rows
                    for q, r in enumerate(rows):
                        b = recs[roff[i] + q]
                        if b["kind"] == F.BEST_NONE:
                            assert r.depth == 0 and r.best_move is None
                            continue
                        want = want_score(int(b["kind"]), int(b["value"]))
                        depth = int(b["pv_len"]) if two else 1
                        assert (r.score, r.depth, r.nodes, r.best_move, r.psqt, r.positional) == \
                            (want, depth, int(b["nodes"]), F.vmove_uci(int(b["move"])), int(b["psqt"]),
                             int(b["positional"])), (NAME[v], two, i, q)
                        mates += want.kind == "mate" and b["kind"] == F.BEST_CP
            assert strip(p1.go(bodies)) != strip(c1.go(bodies))              # without the setting: other answers
        assert mates >= 1
        # the crazyhouse mate behind the drop: after Rxe8+ both blocking drops are taken with mate (Nh6 holds g8)
        body = bodies_of(ZH, [ZH_FORCED])
        assert F.game_end(*ZH_FORCED, ZH) == F.END_CHECK
        row = c1.go(body)[0][1]
        assert row.score == B.Score("mate", -1) and "@" in row.best_move
        assert json.loads(B.into_analysis(c1.go(body)[0]))[1]["score"] == {"mate": -1}
        assert c2.go_pv(body)[0][0].score == B.Score("mate", 2) and c2.go_pv(body)[0][0].best_move == "e1e8"
        assert p1.go(body)[0][1].score.kind == "cp"
        # unchanged: chess batches, move work, depth-0 batches, as on a channel without the setting
        chess = [B.AcquireResponseBody("c0", V.CHESS_START, "e2e4 e7e5 g1f3 b8c6")]
        moves = bodies_of(ZH, SGAMES[ZH][:2], work="move") + bodies_of(AT, SGAMES[AT][:2], work="move")
        assert strip(c1.go(chess + moves)) == strip(p1.go(chess + moves))
        c1.set_variant_analysis_depth(0)
        mixed = chess + bodies_of(ZH, SGAMES[ZH]) + bodies_of(AT, SGAMES[AT])
        assert strip(c1.go(mixed)) == strip(d0.go(mixed))
    finally:
        for _, actor in made:
            actor.close()

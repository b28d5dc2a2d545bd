"""Repetition and fifty-move draws in the variant searches on the device (ABI
3.16), bit-exact: the device history against the host's for all five variants,
the four variant searches with the rules on against the host-built reference of
tests/test_vdraws.py field by field, the switches (rules on over games without a
draw, rules off over games with one, each setter on the other kind of context),
the independence of the marks from the chunk cuts and from key collisions
(fresh child processes), the draws under the atomic quiescence, and the engine
actor beside a chess batch and a batch of another variant."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import backend as B
from tests import test_draws as CD
from tests import test_gpu_vsearch2 as GV
from tests import test_vdraws as D
from tests.conftest import ROOT, net_bytes
from tests.test_gpu_multipv2 import lines_of, want_line

pytestmark = pytest.mark.gpu

ZH, AT, KOTH, RK, TC = D.ZH, D.AT, D.KOTH, D.RK, D.TC
VARIANTS = D.VARIANTS
K = 3
MIN_RECORDS = 219 * 219
# 121 plies each, every one after the 8th with a third occurrence below it; crazyhouse walks the whole game
LONG = {v: (D.START[v], " ".join([D.SHUFFLE[v]] * 30)) for v in (ZH, AT)}
as_tuples = CD.as_tuples


def make(v, draws):
    e = F.Evaluator(F.Net.from_bytes_variant(D.net_data(v), D.net_variant(v)), 0)
    if draws:
        assert e.search_vdraws() is False
        e.set_search_vdraws(True)
        assert e.search_vdraws() is True
    return e


@pytest.fixture(scope="module")
def evs():
    """Contexts that never heard of the setting: a crazyhouse one and an atomic one (which serves the rest)."""
    made = {v: make(v, False) for v in (ZH, AT)}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def ons():
    made = {v: make(v, True) for v in (ZH, AT)}
    yield made
    for e in made.values():
        e.close()


def serving(ctxs, v):
    return ctxs[D.net_variant(v)]


def results(e, v, games):
    """Every variant search of `games` on one context -> {name: array}."""
    s1, off = e.vsearch1(v, games)
    _, _, l1 = e.vsearch1_lines(v, games, K)
    s2, _, kb, km = e.vsearch2(v, games, children=True)
    s2b, _, l2 = e.vsearch2_lines(v, games, K)
    assert s2b.tobytes() == s2.tobytes()
    return {"off": off, "s1": s1, "l1": l1, "s2": s2, "l2": l2, "kb": kb, "km": km}


@pytest.fixture(scope="module")
def searched(ons, evs):
    """Per variant: DRAW_GAMES with the rules on and off (computed once, never changed)."""
    return {v: (results(serving(ons, v), v, D.DRAW_GAMES[v]), results(serving(evs, v), v, D.DRAW_GAMES[v]))
            for v in VARIANTS}


def padded(lines, k, width):
    return [lines[j] if j < len(lines) else (0,) * width for j in range(k)]


# ---- 1. the history ----

@pytest.mark.parametrize("v", VARIANTS)
def test_device_history_equals_the_host(evs, v):
    games = D.HISTORY_GAMES[v] + D.DRAW_GAMES[v] + GV.GAMES[v] + [(D.START[v], ""), (D.START[v], D.SHUFFLE[v].split()[0])]
    if v in LONG:
        games = games + [LONG[v]]
    want, woff = F.game_vhistory(v, games)
    for e in evs.values():  # any net's context serves
        got, off = e.game_vhistory(v, games)
        assert off.tolist() == woff.tolist() and got.tobytes() == want.tobytes()
    assert int(got["seen"].max()) >= 2 and (v == ZH) == (int(got["clock"].max()) == 0)
    none, noff = evs[AT].game_vhistory(v, [])
    assert len(none) == 0 and noff.tolist() == [0]


def test_device_history_errors(evs):
    with pytest.raises(F.FnnueError) as err:
        evs[ZH].game_vhistory(AT, [(D.CHESS_START, "e2e4"), (D.CHESS_START, "e2e4 e2e4")])
    assert err.value.code == D.E_MOVE and "game 1" in str(err.value)
    for variant in (0, 6):
        with pytest.raises(F.FnnueError) as err:
            evs[AT].game_vhistory(variant, [(D.CHESS_START, "")])
        assert err.value.code == D.E_ARG


# ---- 2. the searches with the rules on ----

@pytest.mark.parametrize("v", VARIANTS)
def test_searches_with_draws_against_the_reference(searched, v):
    got, plain = searched[v]
    ref = D.reference(v)
    games = D.DRAW_GAMES[v]
    off = got["off"]
    assert off.tolist() == plain["off"].tolist() == np.cumsum([0] + [len(m.split()) + 1 for _, m in games]).tolist()
    s1, s2 = as_tuples(got["s1"], F.BEST_DTYPE), as_tuples(got["s2"], F.BEST2_DTYPE)
    last_of = {game: int(off[i + 1]) - 1 for i, game in enumerate(games)}
    compared = 0
    for i, (one, lines1, two, lines2, marked, marked2, _) in enumerate(ref):
        p = int(off[i + 1]) - 1
        assert s1[p] == one, (i, dict(zip(F.BEST_DTYPE.names, s1[p])), dict(zip(F.BEST_DTYPE.names, one)))
        assert as_tuples(got["l1"][p], F.LINE_DTYPE) == padded(lines1, K, 7), i
        assert s2[p] == two, (i, dict(zip(F.BEST2_DTYPE.names, s2[p])), dict(zip(F.BEST2_DTYPE.names, two)))
        assert as_tuples(got["l2"][p], F.LINE2_DTYPE) == padded(lines2, K, 10), i
        # The plies above the last.  A third occurrence below ply q needs an identity that stands twice among
        # the plies 0..q, i.e. a ply up to q that has been seen before, and a clock of 100 needs 98 at ply q:
        # without either nothing below q can be drawn and its records are the rules-off bytes.  A ply that is
        # the last ply of a shorter cut of the same game has that cut's records (the same history).
        fen, mv = games[i]
        hist = D.tracked_history(v, [games[i]])[0]
        for q in range(p - int(off[i])):
            clean = all(h[1] == 0 for h in hist[:q + 1]) and hist[q][0] < 98
            shorter = last_of.get((fen, " ".join(mv.split()[:q])))
            for name in ("s1", "l1", "s2", "l2"):
                if clean:
                    assert got[name][int(off[i]) + q].tobytes() == plain[name][int(off[i]) + q].tobytes(), (i, q, name)
                elif shorter is not None:
                    assert got[name][int(off[i]) + q].tobytes() == got[name][shorter].tobytes(), (i, q, name)
            compared += clean or shorter is not None
    assert compared >= 15
    # nodes never change; the rules do change answers
    assert got["s1"]["nodes"].tolist() == plain["s1"]["nodes"].tolist()
    assert got["s2"]["nodes"].tolist() == plain["s2"]["nodes"].tolist()
    assert got["l2"].tobytes() != plain["l2"].tobytes()


def test_what_the_rules_answer(searched):
    last = lambda v, i: int(searched[v][0]["off"][i + 1]) - 1
    # kingOfTheHill with clock 99: g6h6 mates and is not drawn, every other move is worth 0
    got, _ = searched[KOTH]
    k99 = got["s2"][last(KOTH, D.I_KRK[KOTH][0])]
    assert (int(k99["kind"]), F.vmove_uci(int(k99["move"])), int(k99["pv_len"])) == (F.BEST_MATE, "g6h6", 1)
    assert [int(x) for x in got["l1"][last(KOTH, D.I_KRK[KOTH][0])]["value"][1:]] == [0, 0]
    # crazyhouse with clock 99: nothing is drawn
    got, plain = searched[ZH]
    p = last(ZH, D.I_ZH_KRK)
    for name in ("s1", "l1", "s2", "l2"):
        assert got[name][p].tobytes() == plain[name][p].tobytes(), name
    for i in (D.I_ZH8, D.I_ZH9):
        assert got["l2"][last(ZH, i)].tobytes() == plain["l2"][last(ZH, i)].tobytes()
    for i in (D.I_ZH18, D.I_ZH19):
        assert got["kb"].tobytes() != plain["kb"].tobytes()
    # threeCheck: the queen's shuffle marks nothing, kingOfTheHill's marks e7e8
    got, plain = searched[TC]
    assert got["l2"][last(TC, D.I_QK7)].tobytes() == plain["l2"][last(TC, D.I_QK7)].tobytes()
    got, plain = searched[KOTH]
    assert got["l1"][last(KOTH, D.I_QK7)].tobytes() != plain["l1"][last(KOTH, D.I_QK7)].tobytes()


def test_the_drawn_crazyhouse_child_carries_its_own_terms(ons, evs, searched):
    """fnnue_vsearch2_children: the drawn child d6e5 of ply 19 holds its own terms, every other field as searched."""
    got, plain = searched[ZH]
    p = int(got["off"][D.I_ZH19 + 1]) - 1
    km = got["km"].tolist()
    assert km == plain["km"].tolist()
    differ = [d for d in range(len(km)) if km[d][0] == p and got["kb"][d].tobytes() != plain["kb"][d].tobytes()]
    assert len(differ) == 1  # among ply 19's children only the drawn one
    d = differ[0]
    want = D.reference(ZH)[D.I_ZH19][6]["d6e5"]
    assert as_tuples(got["kb"][d:d + 1], F.BEST_DTYPE)[0] == want
    after = (D.ZH_CAP[0], D.ZH_CAP[1])  # the position after d6e5
    ps, po = evs[ZH].eval_vpositions(F.game_vpositions(ZH, *after)[-1:])
    assert (int(got["kb"][d]["psqt"]), int(got["kb"][d]["positional"])) == (int(ps[0]), int(po[0]))
    for name in ("value", "nodes", "best", "move", "kind", "end"):
        assert got["kb"][d][name] == plain["kb"][d][name]


# ---- 3. the switches ----

@pytest.mark.parametrize("v", VARIANTS)
def test_vdraws_on_marks_nothing_on_games_without_a_draw(ons, evs, v):
    a, b = results(serving(ons, v), v, GV.GAMES[v]), results(serving(evs, v), v, GV.GAMES[v])
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_vdraws_off_equals_a_context_never_set(ons, searched):
    for v in (ZH, KOTH):
        on = serving(ons, v)
        on.set_search_vdraws(False)
        try:
            back = results(on, v, D.DRAW_GAMES[v])
        finally:
            on.set_search_vdraws(True)
        for name in back:
            assert back[name].tobytes() == searched[v][1][name].tobytes(), (v, name)


def test_each_setter_is_ignored_by_the_other_kind_of_context(evs, searched):
    e = evs[AT]
    e.set_search_draws(True)  # chess's setter on a variant context: nothing changes
    try:
        back = results(e, AT, D.DRAW_GAMES[AT])
    finally:
        e.set_search_draws(False)
    for name in back:
        assert back[name].tobytes() == searched[AT][1][name].tobytes(), name
    chess = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
    try:
        games = CD.DRAW_GAMES
        before = (chess.search2(games)[0].tobytes(), chess.search1_lines(games, K)[2].tobytes())
        chess.set_search_vdraws(True)  # the variants' setter on a chess context
        assert chess.search_vdraws() is True and chess.search_draws() is False
        assert (chess.search2(games)[0].tobytes(), chess.search1_lines(games, K)[2].tobytes()) == before
    finally:
        chess.close()


# ---- 4. chunk cuts and key collisions: fresh child processes ----

CHILD = """
import sys
import numpy as np
import fishnet_amd as F
from tests import test_gpu_vsearch2 as GV
from tests import test_vdraws as D
from tests.test_gpu_vdraws import LONG, make, results
out = {}
for v in LONG:
    ev = make(v, True)
    out.update({"a%d_" % v + k: a for k, a in results(ev, v, D.DRAW_GAMES[v] + [LONG[v]]).items()})
    out.update({"b%d_" % v + k: a for k, a in results(ev, v, GV.GAMES[v][:3]).items()})
    out["hist%d" % v], out["hoff%d" % v] = ev.game_vhistory(v, D.HISTORY_GAMES[v] + [LONG[v]])
    ev.close()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def in_process(ons):
    out = {}
    for v in LONG:
        on = ons[v]
        out.update({"a%d_" % v + k: a for k, a in results(on, v, D.DRAW_GAMES[v] + [LONG[v]]).items()})
        out.update({"b%d_" % v + k: a for k, a in results(on, v, GV.GAMES[v][:3]).items()})
        out["hist%d" % v], out["hoff%d" % v] = on.game_vhistory(v, D.HISTORY_GAMES[v] + [LONG[v]])
    return out


@pytest.mark.parametrize("env", [{"FNNUE_SEARCH2_RECORDS": str(MIN_RECORDS)}, {"FNNUE_DRAW_KEY_BITS": "4"}],
                         ids=["chunks", "collisions"])
def test_results_do_not_depend_on_chunks_or_key_collisions(in_process, evs, tmp_path, env):
    for v in LONG:
        nodes = in_process["a%d_s2" % v]["nodes"].astype(np.int64)
        assert nodes.max() <= MIN_RECORDS and nodes.sum() > MIN_RECORDS and nodes.sum() < 16 << 20  # several chunks
        assert (in_process["hist%d" % v]["seen"] >= 2).sum() > 100
        plain = results(evs[v], v, [LONG[v]])  # at least one record is marked: the answers differ from rules off
        n = len(plain["s2"])
        assert in_process["a%d_l2" % v][-n:].tobytes() != plain["l2"].tobytes()
    path = str(tmp_path / "child.npz")
    subprocess.run([sys.executable, "-c", CHILD, path], cwd=ROOT, env=dict(os.environ, **env), check=True, timeout=300)
    child = np.load(path)
    assert sorted(child.files) == sorted(in_process)
    for name in child.files:
        assert child[name].tobytes() == in_process[name].tobytes(), name


# ---- 5. under the quiescence ----

def test_a_drawn_leaf_is_not_quiesced(ons, searched):
    """Atomic, quiescence depth 1 with checks together with the draws: the marks are set before the tree, a drawn
    leaf is skipped by it and keeps its place and its value 0."""
    games = D.DRAW_GAMES[AT]
    on = ons[AT]
    on.set_search_vquiesce(1, True)
    try:
        q = results(on, AT, games)
    finally:
        on.set_search_vquiesce(0, False)
    got, _ = searched[AT]
    ref = D.reference(AT)
    for i in (D.I_CUT7, D.I_KRK[AT][0], D.I_KRK[AT][2]):  # a repetition, and the clocks 99 and 120
        p = int(got["off"][i + 1]) - 1
        lines1, marked = ref[i][1], ref[i][4]
        n1 = len(lines1)
        full = on.vsearch1_lines(AT, games, n1)[2][p]  # without the quiescence, every child
        on.set_search_vquiesce(1, True)
        try:
            qfull = on.vsearch1_lines(AT, games, n1)[2][p]
        finally:
            on.set_search_vquiesce(0, False)
        drawn = {D.vcode_of(t) for t in marked}
        assert drawn
        for lines in (full, qfull):
            at = {int(l["move"]): l for l in lines}
            for code in drawn:
                assert (int(at[code]["value"]), int(at[code]["kind"])) == (0, F.BEST_CP)
        for code in drawn:  # untouched by the tree: the terms of the record itself
            a, b = {int(l["move"]): l for l in full}[code], {int(l["move"]): l for l in qfull}[code]
            assert (int(a["psqt"]), int(a["positional"])) == (int(b["psqt"]), int(b["positional"]))
    assert q["s2"]["nodes"].tolist() == got["s2"]["nodes"].tolist()


# ---- 6. the engine actor ----

ACTOR = {ZH: [D.DRAW_GAMES[ZH][D.I_ZH19], D.DRAW_GAMES[ZH][D.I_CUT7]],
         AT: [D.DRAW_GAMES[AT][D.I_CUT7], D.DRAW_GAMES[AT][D.I_KRK[AT][0]], GV.GAMES[AT][0]]}


@pytest.fixture(scope="module")
def chans():
    """(2 variant and chess plies with the variants' draw rules, the same without, never set): all six nets."""
    made = []
    for kw in ({"variant_analysis_plies": 2, "analysis_plies": 2, "variant_draw_rules": True},
               {"variant_analysis_plies": 2, "analysis_plies": 2}, {}):
        chess, vnets = GV.nets()
        made.append(B.channel(chess, 0, **vnets, **kw))
    yield tuple(stub for stub, _ in made)
    for _, actor in made:
        actor.close()


def test_actor_with_variant_draw_rules(chans, ons):
    dd, d2, d0 = chans
    assert dd.variant_draw_rules() is True and d2.variant_draw_rules() is False and dd.draw_rules() is False
    chess_bodies = [B.AcquireResponseBody("chess0", *CD.DRAW_GAMES[CD.I_CUT7]),
                    B.AcquireResponseBody("chess1", *CD.DRAW_GAMES[CD.I_K99])]
    bodies = {v: GV.bodies_of(v, ACTOR[v]) for v in ACTOR}
    everything = bodies[ZH] + chess_bodies + bodies[AT]
    res, zero = dd.go_pv(everything), d0.go(everything)
    lres = dd.go_lines_pv(GV.bodies_of(ZH, ACTOR[ZH], multipv=K) + chess_bodies + GV.bodies_of(AT, ACTOR[AT], multipv=K))
    part = {ZH: (0, len(bodies[ZH])), AT: (len(bodies[ZH]) + 2, len(everything))}
    for v, (lo, hi) in part.items():
        want = results(ons[v], v, ACTOR[v])
        off = want["off"]
        for i, (rows, zrows) in enumerate(zip(res[lo:hi], zero[lo:hi])):
            assert not isinstance(rows, B.PositionFailed), rows
            GV.check_two_plies(rows, zrows, want["s2"][off[i]:off[i + 1]])
        got = lines_of(lres[lo:hi])
        for i in range(len(ACTOR[v])):
            for q in range(int(off[i + 1] - off[i])):
                ls = want["l2"][off[i] + q]
                legal = int((ls["kind"] != F.BEST_NONE).sum())
                if legal:
                    assert got[i][q] == [want_line(l, F.vmove_uci) for l in ls[:legal]], (v, i, q)
        # a drawn best move answers as a stalemating one: Cp(0), depth 1, a one-move pv
        drawn_first = [(i, q) for i in range(len(ACTOR[v])) for q, b in enumerate(want["s2"][off[i]:off[i + 1]])
                       if b["kind"] == F.BEST_CP and b["pv_len"] == 1 and b["value"] == 0]
        assert drawn_first or v == ZH
        for i, q in drawn_first:
            r = res[lo + i][q]
            assert (r.score, r.depth, r.reply) == (B.Score("cp", 0), 1, None)
            assert json.loads(B.into_analysis(res[lo + i]))[q]["pv"] == r.best_move
    # the drawn crazyhouse child d6e5 is a one-move line worth 0 wherever it ranks
    zh_last = lines_of(dd.go_lines_pv(GV.bodies_of(ZH, ACTOR[ZH][:1], multipv=500)))[0][-1]
    assert [l[:2] for l in zh_last if l[2] == ("d6e5",)] == [("cp", 0)]
    # the chess batches: as on a channel without the setting; the rules matter for the variants'
    lo = len(bodies[ZH])
    assert GV.strip(res[lo:lo + 2]) == GV.strip(d2.go_pv(chess_bodies))
    assert GV.strip(res[:lo]) != GV.strip(d2.go_pv(bodies[ZH])) or GV.strip(res[lo + 2:]) != GV.strip(d2.go_pv(bodies[AT]))
    # chess's setter does not touch variant batches
    d2.set_draw_rules(True)
    try:
        assert GV.strip(d2.go_pv(bodies[AT])) != GV.strip(res[lo + 2:])
    finally:
        d2.set_draw_rules(False)
    # one ply: fnnue_vsearch1's answers with the rules on
    dd.set_variant_analysis_plies(1)
    try:
        one = dd.go(bodies[AT])
        want = results(ons[AT], AT, ACTOR[AT])
        off = want["off"]
        for i, rows in enumerate(one):
            for r, b in zip(rows, want["s1"][off[i]:off[i + 1]]):
                if b["kind"] in (F.BEST_CP, F.BEST_MATE):
                    assert (r.depth, r.best_move, r.nodes) == (1, F.vmove_uci(int(b["move"])), int(b["nodes"]))
                if b["kind"] == F.BEST_CP:
                    assert r.score == B.Score("cp", GV.trunc_div(int(b["value"]) * 100, GV.NORM))
    finally:
        dd.set_variant_analysis_plies(2)
    # set back to off: a channel that was never set
    dd.set_variant_draw_rules(False)
    try:
        assert dd.variant_draw_rules() is False
        assert GV.strip(dd.go_pv(everything)) == GV.strip(d2.go_pv(everything))
    finally:
        dd.set_variant_draw_rules(True)

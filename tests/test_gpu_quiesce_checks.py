"""Quiescence checks on the device (ABI 3.14), bit-exact and field by field:
fnnue_quiesce with the setting on against the rule Q' in Python
(tests/test_quiesce_checks.py qc_ref) over random games that hold evasions,
mates of both signs and mates met only at the horizon; frontiers of 63 / 64 /
65 expanding nodes; the smallest budgets; the five searches against the
existing reductions over Q'-substituted leaves; the behaviour on the material
net; the setting off, or on with depth 0, byte-identical to a context that
never had it; drawn and NO_MOVES leaves; a variant context; the engine actor
and its mate mapping."""
import json

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import backend as B
from tests import material_net as M
from tests import test_draws as D
from tests import test_multipv2 as M2
from tests import test_quiesce as Q
from tests import test_quiesce_checks as QC
from tests import test_search2 as R
from tests.conftest import net_bytes
from tests.test_gpu_multipv2 import make_channel
from tests.test_gpu_quiesce import K, SCANDI, env, ordered_lines1, plies_of, results, same
from tests.test_gpu_search1 import NORM
from tests.test_gpu_search2 import ZH, ZH_START, as_tuples, bodies_of, strip, trunc_div

pytestmark = pytest.mark.gpu

START = Q.START
# random games (at most 24 plies) from the start, a middlegame and three heavy-piece endings with back-rank
# mates about; the seeds were chosen on the host so that the reference holds what
# test_reference_holds_what_the_issue_asks asserts
KIWI = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
BACK = "r5k1/5ppp/8/8/8/8/5PPP/R5K1 w - - 0 1"
QQ = "3q2k1/5ppp/8/8/8/8/5PPP/3Q2K1 w - - 0 1"
RRQQ = "r2q2k1/5ppp/8/8/8/8/5PPP/R2Q2K1 w - - 0 1"
SEEDS = [(BACK, 7), (BACK, 8), (BACK, 51), (QQ, 6), (QQ, 30), (RRQQ, 2), (RRQQ, 22), (RRQQ, 57), (KIWI, 4), (START, 5)]
RGAMES = [(fen, F.random_game(seed, fen, 24)) for fen, seed in SEEDS]

SKEWER_B = "4k3/8/8/8/8/8/r7/4K2Q b - - 0 1"        # ...Ra1+ skewers the queen
MATE_BEHIND = "6k1/5ppp/r7/8/8/8/8/R3K3 b - - 0 1"   # ...Ra8 walks into Rxa8 mate
MATE3 = "r4k2/5ppp/8/B7/8/8/8/R3R1K1 w - - 0 1"      # Bb4+ opens the a-file: Kg8 (forced) Rxa8 mate
SGAMES = [(QC.CHAIN, ""), (QC.CAPTURE_MATE, ""), (QC.SKEWER, ""), (MATE_BEHIND, ""), (SKEWER_B, ""), (Q.IN_CHECK, ""),
          (R.MATE_OR_STALEMATE, ""), (MATE3, "")]


@pytest.fixture(scope="module")
def data():
    return net_bytes(1, 256, 0)


@pytest.fixture(scope="module")
def ev(data):
    """A context that never heard of the setting."""
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ce(data):
    """A context with the setting on (the tests that turn it off put it back)."""
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    assert not e.search_quiesce_checks()
    e.set_search_quiesce_checks(True)
    assert e.search_quiesce_checks()
    yield e
    e.close()


@pytest.fixture(scope="module")
def ce128():
    e = F.Evaluator(F.Net.from_bytes(net_bytes(1, 128, 0)), 0)
    e.set_search_quiesce_checks(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mat():
    e = F.Evaluator(F.Net.from_bytes(M.material_net(128)), 0)
    yield e
    e.close()


_QREF = {}


def checks_reference(hd):
    """qc_ref of every ply of RGAMES for d = 0..3 with what it met (computed once per net, shared)."""
    if hd not in _QREF:
        o, stats = Q.OracleNet(net_bytes(1, hd, 0)), {}
        _QREF[hd] = ({d: [QC.qc_ref(o, fen, mv, d, stats=stats) for fen, mv in plies_of(RGAMES)] for d in range(4)},
                     stats)
    return _QREF[hd]


_SREF = {}


def searches_reference(data, d):
    if d not in _SREF:
        _SREF[d] = QC.search_reference(data, SGAMES, d)
    return _SREF[d]


def with_quiesce(e, d, fn):
    e.set_search_quiesce(d)
    try:
        return fn()
    finally:
        e.set_search_quiesce(0)


# ---- 1. fnnue_quiesce against the rule ----

@pytest.mark.parametrize("hd", [256, 128])
def test_reference_holds_what_the_issue_asks(hd):
    ref, stats = checks_reference(hd)
    assert all(len(mv.split()) <= 24 for _, mv in RGAMES)
    assert stats["in_check"] >= 20                                   # nodes in check that listed evasions
    assert stats["horizon_mates"] >= 1                               # a mate met only at the horizon
    decided = [r[2] for d in range(4) for r in ref[d] if r[6]]
    assert sum(v > 0 for v in decided) >= 5 and sum(v < 0 for v in decided) >= 5
    assert stats["max_static"] < QC.DOMAIN                           # the rule's domain
    assert any(r[6] and r[5] >= 2 for r in ref[3])                   # a mate more than one ply away
    assert sum(r[3] for d in range(4) for r in ref[d]) < 60000       # the trees stay small


@pytest.mark.parametrize("hd", [256, 128])
def test_quiesce_with_checks_matches_the_rule(ce, ce128, hd):
    e = ce if hd == 256 else ce128
    ref, _ = checks_reference(hd)
    woff = np.cumsum([0] + [len(mv.split()) + 1 for _, mv in RGAMES])
    plies = plies_of(RGAMES)
    for d in range(4):
        got, off = e.quiesce(RGAMES, d)
        assert off.tolist() == woff.tolist() and len(got) == len(ref[d])
        for p, (g, w) in enumerate(zip(QC.quiet_tuples(got), ref[d])):
            assert g == w, (d, p, plies[p])


def test_quiesce_with_checks_on_the_rule_cases(mat):
    o = Q.material_oracle()
    games = [(QC.SKEWER, ""), (QC.CAPTURE_MATE, "a1a8"), (QC.CHAIN, "f8g8 a1a8"), (MATE3, "a5b4")]
    mat.set_search_quiesce_checks(True)
    try:
        for d in range(5):
            got, _ = mat.quiesce(games, d)
            want = [QC.qc_ref(o, fen, mv, d) for fen, mv in plies_of(games)]
            assert QC.quiet_tuples(got) == want, d
        got, _ = mat.quiesce(games, 2)
    finally:
        mat.set_search_quiesce_checks(False)
    plain, _ = mat.quiesce(games, 2)
    assert not plain["reserved"].any() and got.tobytes() != plain.tobytes()
    values = got["value"].tolist()
    assert values[0] == M.balance(QC.SKEWER) - 900 and int(plain["value"][0]) == M.balance(QC.SKEWER)
    assert values[1:3] == [31999, -32000] and values[3:6] == [-31998, 31999, -32000]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_a_frontier_of_63_64_65_nodes_in_check(ce, n):
    game = (SKEWER_B, "a2a1")                       # its last ply is in check with three evasions, the first has no capture
    one, _ = ce.quiesce([game], 3)
    assert int(one["nodes"][0]) == 0 and int(one["nodes"][1]) > 3 and int(one["len"][1]) >= 2
    got, _ = ce.quiesce([game] * n, 3)
    assert len(got) == 2 * n and got.tobytes() == np.tile(one, n).tobytes()


def test_results_do_not_depend_on_the_budgets(ce):
    games = RGAMES[:6]
    want, _ = ce.quiesce(RGAMES, 3)
    wres = with_quiesce(ce, 2, lambda: results(ce, games))
    with env(FNNUE_QUIESCE_RECORDS=256, FNNUE_SEARCH2_RECORDS=1):
        before = ce.quiesce_slices()
        got, _ = ce.quiesce(RGAMES, 3)
        assert ce.quiesce_slices() - before > 1
        gres = with_quiesce(ce, 2, lambda: results(ce, games))
    assert got.tobytes() == want.tobytes() and same(gres, wres)


# ---- 2. the searches against the existing reductions over Q'-substituted leaves ----

@pytest.mark.parametrize("d", [1, 2])
def test_searches_match_the_reference_with_substituted_leaves(data, ce, d):
    ref = searches_reference(data, d)
    got = with_quiesce(ce, d, lambda: results(ce, SGAMES))
    s1, s2 = as_tuples(got["s1"], F.BEST_DTYPE), as_tuples(got["s2"], F.BEST2_DTYPE)
    assert len(s1) == len(s2) == len(ref)
    kbt, kid = as_tuples(got["kb"], F.BEST_DTYPE), 0
    coded = 0
    for p, r in enumerate(ref):
        assert s1[p] == r["one"], (p, s1[p], r["one"])
        assert s2[p] == r["two"], (p, s2[p], r["two"])
        want1 = ordered_lines1(*r["group"])[:K]
        got1 = as_tuples(got["l1"][p][:len(want1)], F.LINE_DTYPE)
        assert got1 == want1, (p, got1, want1)
        end, codes = r["group"][2], r["group"][3]
        want2 = M2.ordered_lines(end, codes, r["cb"], False)[:K]
        got2 = as_tuples(got["l2"][p][:len(want2)], F.LINE2_DTYPE)
        assert got2 == want2, (p, got2, want2)
        for cb in r["cb"]:  # the children's own depth-1 records
            if cb[R.BEST["kind"]] != F.BEST_NONE:
                assert kbt[kid] == cb, (p, kid)
            kid += 1
        coded += abs(r["one"][R.BEST["value"]]) > QC.DOMAIN
        coded += abs(r["two"][R.B2["value"]]) > QC.DOMAIN
    assert kid == len(kbt) and coded >= 2            # coded mates did reach the reductions
    # the forced line of MATE3 at two plies: Bb4+ Kg8 and the mate one ply below the leaf
    two = ref[len(SGAMES) - 1]["two"]
    assert (two[R.B2["value"]], two[R.B2["kind"]], F.move_uci(two[R.B2["move"]])) == (31997, F.BEST_CP, "a5b4")


# ---- 3. behaviour on the material net ----

def test_one_ply_finds_the_skewer(mat):
    def run(on):
        mat.set_search_quiesce_checks(on)
        try:
            return with_quiesce(mat, 2, lambda: mat.search1_lines([(SKEWER_B, "")], 218))
        finally:
            mat.set_search_quiesce_checks(False)

    (off, _, loff), (on, _, lon) = run(False), run(True)
    bal = M.balance(SKEWER_B)                        # a rook against a queen: -400
    assert F.move_uci(int(on["move"][0])) == "a2a1" and int(on["value"][0]) == bal + 900
    assert int(off["value"][0]) <= int(on["value"][0]) - 900
    skewer = lambda rows: next(r for r in rows[0] if F.move_uci(int(r["move"])) == "a2a1")
    assert int(skewer(loff)["value"]) == bal         # the plain rule lets the side in check stand pat: no gain there


def test_one_ply_sees_the_mate_behind_the_capture(mat):
    mat.set_search_quiesce_checks(True)
    try:
        best, _, lines = with_quiesce(mat, 1, lambda: mat.search1_lines([(MATE_BEHIND, "")], 218))
    finally:
        mat.set_search_quiesce_checks(False)
    row = next(r for r in lines[0] if F.move_uci(int(r["move"])) == "a6a8")
    assert (int(row["value"]), int(row["kind"]), int(row["psqt"]), int(row["positional"])) == \
        (-31998, F.BEST_CP, 0, -16 * 31998)
    assert F.move_uci(int(best["move"][0])) != "a6a8" and abs(int(best["value"][0])) < QC.DOMAIN
    stub, actor = B.channel(F.Net.from_bytes(M.material_net(128)), 0, analysis_depth=1, quiesce=1,
                            quiesce_checks=True)
    try:
        assert stub.quiesce_checks()
        rows = stub.go_lines(bodies_of([(MATE_BEHIND, "")], multipv=500))[0]
        line = next(l for l in rows[0].lines if l.move == "a6a8")
        assert line.score == B.Score("mate", -1)
        assert rows[0].score.kind == "cp"
    finally:
        actor.close()


# ---- 4. the setting off, or on with depth 0 ----

def test_setting_off_and_depth_zero_are_byte_identical(ev, ce):
    games = SGAMES + RGAMES[:3]
    plain0 = results(ev, games)
    assert same(results(ce, games), plain0)                      # on, with depth 0
    plain2 = with_quiesce(ev, 2, lambda: results(ev, games))
    pq, _ = ev.quiesce(RGAMES, 2)
    assert not pq["reserved"].any()
    on2 = with_quiesce(ce, 2, lambda: results(ce, games))
    assert not same(on2, plain2)                                 # the setting does reach the leaves
    ce.set_search_quiesce_checks(False)
    try:
        off2 = with_quiesce(ce, 2, lambda: results(ce, games))
        oq, _ = ce.quiesce(RGAMES, 2)
    finally:
        ce.set_search_quiesce_checks(True)
    assert same(off2, plain2) and oq.tobytes() == pq.tobytes()


# ---- 5. drawn and NO_MOVES leaves ----

def test_drawn_and_final_leaves_stay_untouched(ce):
    games = [(D.START, " ".join([D.SHUFFLE] * 2)), (D.START, "e2e4 d7d5 " + " ".join([D.SHUFFLE] * 2)),
             (QC.CAPTURE_MATE, ""), (R.MATE_OR_STALEMATE, "")]

    def lines(draws, d):
        ce.set_search_draws(draws)
        try:
            best, _, ls = with_quiesce(ce, d, lambda: ce.search1_lines(games, 218))
        finally:
            ce.set_search_draws(False)
        return [{int(r["child"]): (int(r["psqt"]), int(r["positional"]), int(r["value"]), int(r["kind"]), int(r["move"]))
                 for r in ls[p][ls[p]["kind"] != F.BEST_NONE]} for p in range(len(best))]

    plain, drawn, quiet, both = lines(False, 0), lines(True, 0), lines(False, 2), lines(True, 2)
    prefixes = plies_of(games)
    marked = final = 0
    for p in range(len(plain)):
        assert set(plain[p]) == set(both[p])
        for c in plain[p]:
            if drawn[p][c] != plain[p][c]:       # a drawn leaf: worth 0, and left alone by the quiescence
                marked += 1
                assert both[p][c] == drawn[p][c] and both[p][c][2] == 0
            else:
                assert both[p][c] == quiet[p][c]
            after = (prefixes[p][1] + " " + F.move_uci(plain[p][c][4])).strip()
            if F.game_end(prefixes[p][0], after) & F.END_NO_MOVES:   # mate or stalemate: never a root of the tree
                final += 1
                assert quiet[p][c] == plain[p][c]
    assert marked >= 2 and final >= 4            # Rxa8 mate; Qg7 and Qf8 mate, Kg6 stalemates


# ---- 6. a variant context ----

def test_variant_context_accepts_and_ignores_the_setting():
    zh = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, 256, ZH), ZH), 0)
    try:
        games = [(ZH_START, "e2e4 d7d5 e4d5 d8d5")]
        zh.set_search_quiesce(2)
        a1, _ = zh.vsearch1(ZH, games)
        a2 = zh.vsearch2(ZH, games)[0]
        zh.set_search_quiesce_checks(True)
        assert zh.search_quiesce_checks()
        b1, _ = zh.vsearch1(ZH, games)
        b2 = zh.vsearch2(ZH, games)[0]
        assert a1.tobytes() == b1.tobytes() and a2.tobytes() == b2.tobytes()
    finally:
        zh.close()


# ---- 7. the actor ----

def want_score(kind, value):
    """The actor's answer to a best / line record under the setting."""
    if kind == F.BEST_MATE:
        return B.Score("mate", 1)
    if kind in (F.BEST_MATED, F.BEST_LOST):
        return B.Score("mate", -1)
    if abs(value) > QC.DOMAIN:
        plies = QC.MATE - abs(value)
        return B.Score("mate", (plies + 1) // 2 if value > 0 else -(plies // 2))
    return B.Score("cp", trunc_div(value * 100, NORM))


def test_actor_with_every_search_setting_matches_the_library(data):
    """The draw rules, quiescence 1 with checks and MultiPV lines at two plies, all on at once: the actor's
    answers and lines against search2_lines, record for record (both run the same level-2 steps)."""
    games = [(D.START, " ".join([D.SHUFFLE] * 2)),                      # a threefold repetition in reach
             (START, "f2f3 e7e5 g2g4 d8h4"),                            # ends in mate
             ("7k/5Q2/5K2/8/8/8/8/8 w - - 0 1", "f6g6"),                # ends in stalemate
             SCANDI]                                                    # captures and checks about
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    stub, actor = make_channel(data, draw_rules=True, quiesce=1, quiesce_checks=True, analysis_plies=2)
    try:
        e.set_search_draws(True)
        e.set_search_quiesce(1)
        e.set_search_quiesce_checks(True)
        out, off, l2 = e.search2_lines(games, K)
        n0 = off[1]   # the shuffle game's plies: the repetition is in reach, so the draw rules change their answers
        e.set_search_draws(False)
        assert e.search2_lines(games, K)[2][:n0].tobytes() != l2[:n0].tobytes()
        e.set_search_draws(True)
        res = stub.go_lines_pv(bodies_of(games, multipv=K))
        uci = lambda m: F.move_uci(int(m))
        ended = 0
        for i, rows in enumerate(res):
            assert not isinstance(rows, B.PositionFailed), rows
            assert len(rows) == off[i + 1] - off[i]
            for q, r in enumerate(rows):
                b, ls = out[off[i] + q], l2[off[i] + q]
                if b["kind"] == F.BEST_NONE:
                    ended += 1
                    assert r.depth == 0 and r.best_move is None and not r.lines
                    continue
                want = want_score(int(b["kind"]), int(b["value"]))
                assert (r.score, r.depth, r.nodes, r.best_move, r.psqt, r.positional) == \
                    (want, int(b["pv_len"]), int(b["nodes"]), uci(b["move"]), int(b["psqt"]), int(b["positional"]))
                legal = ls[ls["kind"] != F.BEST_NONE]
                assert 1 <= len(legal) <= K
                assert [(l.score, tuple(l.pv), l.psqt, l.positional) for l in r.lines] == \
                    [(want_score(int(l["kind"]), int(l["value"])),
                      (uci(l["move"]),) + ((uci(l["reply"]),) if int(l["pv_len"]) == 2 else ()),
                      int(l["psqt"]), int(l["positional"])) for l in legal]
        assert ended == 2   # the mated and the stalemated last plies
    finally:
        actor.close()
        e.close()


def test_actor_with_quiescence_checks_matches_the_library(data, ce):
    made = [make_channel(data, quiesce=1, quiesce_checks=True, analysis_depth=1),
            make_channel(data, quiesce=1, quiesce_checks=True, analysis_plies=2),
            make_channel(data, quiesce=1, analysis_depth=1), make_channel(data)]
    try:
        (c1, c2, q1, d0) = (stub for stub, _ in made)
        assert c1.quiesce_checks() and not q1.quiesce_checks() and not d0.quiesce_checks()
        games = SGAMES + [SCANDI]
        bodies = bodies_of(games, multipv=K)

        def library():
            best, goff, l1 = ce.search1_lines(games, K)
            out, off, l2 = ce.search2_lines(games, K)
            return best, goff, l1, out, off, l2

        best, goff, l1, out, off, l2 = with_quiesce(ce, 1, library)
        mates = {"go": 0, "go_lines": 0, "go_pv": 0, "go_lines_pv": 0}
        res1 = c1.go_lines(bodies)
        assert strip(c1.go(bodies)) == strip(res1)
        for i, rows in enumerate(res1):
            assert not isinstance(rows, B.PositionFailed), rows
            for q, r in enumerate(rows):
                b, ls = best[goff[i] + q], l1[goff[i] + q]
                if b["kind"] == F.BEST_NONE:
                    assert r.depth == 0 and r.best_move is None
                    continue
                want = want_score(int(b["kind"]), int(b["value"]))
                assert (r.score, r.depth, r.nodes, r.best_move, r.psqt, r.positional) == \
                    (want, 1, int(b["nodes"]), F.move_uci(int(b["move"])), int(b["psqt"]), int(b["positional"]))
                mates["go"] += want.kind == "mate" and b["kind"] == F.BEST_CP
                legal = ls[ls["kind"] != F.BEST_NONE]
                assert [(l.score, l.move) for l in r.lines] == \
                    [(want_score(int(l["kind"]), int(l["value"])), F.move_uci(int(l["move"]))) for l in legal]
                mates["go_lines"] += sum(l["kind"] == F.BEST_CP and abs(int(l["value"])) > QC.DOMAIN for l in legal)
        res2 = c2.go_lines_pv(bodies)
        assert strip(c2.go_pv(bodies)) == strip(res2)
        for i, rows in enumerate(res2):
            assert not isinstance(rows, B.PositionFailed), rows
            for q, r in enumerate(rows):
                b, ls = out[off[i] + q], l2[off[i] + q]
                if b["kind"] == F.BEST_NONE:
                    assert r.depth == 0 and r.best_move is None
                    continue
                want = want_score(int(b["kind"]), int(b["value"]))
                assert (r.score, r.depth, r.nodes, r.best_move, r.psqt, r.positional) == \
                    (want, int(b["pv_len"]), int(b["nodes"]), F.move_uci(int(b["move"])), int(b["psqt"]),
                     int(b["positional"]))
                mates["go_pv"] += want.kind == "mate" and b["kind"] == F.BEST_CP
                legal = ls[ls["kind"] != F.BEST_NONE]
                assert [(l.score, l.pv[0]) for l in r.lines] == \
                    [(want_score(int(l["kind"]), int(l["value"])), F.move_uci(int(l["move"]))) for l in legal]
                mates["go_lines_pv"] += sum(l["kind"] == F.BEST_CP and abs(int(l["value"])) > QC.DOMAIN for l in legal)
        assert all(v >= 1 for v in mates.values()), mates
        # the named cases: the forced evasion into the mate at one ply, the forced line at two
        chain, mate3 = games.index((QC.CHAIN, "")), games.index((MATE3, ""))
        assert res1[chain][0].score == B.Score("mate", -1) and res1[chain][0].best_move == "f8g8"
        assert res2[mate3][0].score == B.Score("mate", 2) and res2[mate3][0].best_move == "a5b4"
        # the compact form and the JSON
        compact = lambda res: [[(r.position_id, r.score, r.psqt, r.positional, r.depth) for r in rows] for rows in res]
        assert compact(c1.go_compact(bodies)) == compact(res1) and compact(c2.go_compact(bodies)) == compact(res2)
        assert compact(c1.go_compact(bodies))[chain][0][1] == B.Score("mate", -1)
        assert json.loads(B.into_analysis(c1.go(bodies_of(games))[chain]))[0]["score"] == {"mate": -1}
        assert json.loads(B.into_analysis(c2.go_pv(bodies_of(games))[mate3]))[0]["score"] == {"mate": 2}
        assert json.loads(B.into_analysis(res2[mate3]))[0]["score"][0][-1] == {"mate": 2}   # the lines' matrix
        # without the setting no value is remapped, and the plain quiescence answers
        plain = q1.go(bodies_of(games))
        assert plain[chain][0].score.kind == "cp" and strip(plain) != strip(c1.go(bodies_of(games)))
        # depth-0 analysis, move work and a crazyhouse batch in one call: as on a channel without the settings
        c1.set_analysis_depth(0)
        mixed = bodies_of(games[:3]) + bodies_of(games[3:5], work="move") + \
            [B.AcquireResponseBody("zh", ZH_START, "e2e4 d7d5 e4d5", variant="crazyhouse")]
        assert strip(c1.go(mixed)) == strip(d0.go(mixed))
    finally:
        for _, actor in made:
            actor.close()

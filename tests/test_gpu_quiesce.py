"""Capture quiescence on the device (ABI 3.13), bit-exact and field by field:
fnnue_quiesce against the rule in Python (tests/test_quiesce.py q_ref), the
searches with the setting on against the host-built reference with the leaves'
terms substituted, invariants over the two-ply games without a reference
(quiesce 0 byte-identical to a context that never heard of the setting, the
reported triple consistent, nodes unchanged, slot 0 of the lines the best
record, independence from the chunk cuts and the slices), the behaviour on the
material net, the draw rules beside it, a variant context, and the engine actor."""
import ctypes as C
import os

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from tests import material_net as M
from tests import test_draws as D
from tests import test_multipv2 as M2
from tests import test_quiesce as Q
from tests import test_search2 as R
from tests.conftest import net_bytes
from tests.test_gpu_multipv2 import make_channel
from tests.test_gpu_search1 import check_depth1
from tests.test_gpu_search2 import ZH, ZH_START, as_tuples, bodies_of, check_two_plies, strip

pytestmark = pytest.mark.gpu

START = Q.START
K = 3
# two games of about 8 plies with captures on the board, and a middlegame with a dozen captures per side
SCANDI = (START, "e2e4 d7d5 e4d5 d8d5 b1c3 d5a5 d2d4 g8f6")
SCOTCH = (START, "e2e4 e7e5 g1f3 b8c6 d2d4 e5d4 f3d4 c6d4 d1d4")
TENSE = ("r1bq1rk1/ppp2ppp/2np1n2/2b1p1B1/2B1P3/2NP1N2/PPP2PPP/R2Q1RK1 w - - 0 1", "c3d5 c6d4")
KIWI = ("r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", "e2a6 b4c3 d2c3")
PROMO5 = ("rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8", "")   # d7xc8 promotes with a capture
QGAMES = Q.HAND_MADE + [SCANDI, SCOTCH, TENSE, KIWI, PROMO5, (START, "g1f3 g8f6")]
# low-piece plies for the searches' reference
SGAMES = [(Q.HANGS, ""), (Q.TRADE, ""), Q.EP, (Q.PROMO, ""), (Q.IN_CHECK, ""), (Q.FLIP, ""), (R.MATE_OR_STALEMATE, "")]


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
def qe(data):
    """A context whose setting the tests change (and put back to 0)."""
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    assert e.search_quiesce() == 0
    yield e
    e.close()


@pytest.fixture(scope="module")
def mat():
    e = F.Evaluator(F.Net.from_bytes(M.material_net(128)), 0)
    yield e
    e.close()


def plies_of(games):
    return [(fen, " ".join(mv.split()[:q])) for fen, mv in games for q in range(len(mv.split()) + 1)]


_QREF = {}


def quiet_reference(data_key, data, games):
    """q_ref of every ply of `games` for d = 0..3 (computed once per net, shared)."""
    if data_key not in _QREF:
        o = Q.OracleNet(data)
        _QREF[data_key] = {d: [Q.q_ref(o, fen, mv, d) for fen, mv in plies_of(games)] for d in range(4)}
    return _QREF[data_key]


def results(e, games):
    s1, off = e.search1(games)
    _, _, l1 = e.search1_lines(games, K)
    s2, _, kb, km = e.search2(games, children=True)
    s2b, _, l2 = e.search2_lines(games, K)
    assert s2b.tobytes() == s2.tobytes()
    return {"off": off, "s1": s1, "l1": l1, "s2": s2, "l2": l2, "kb": kb, "km": km}


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- 1. fnnue_quiesce against the rule ----

def test_reference_holds_what_the_issue_asks(data):
    ref = quiet_reference("rnd", data, QGAMES)
    mref = quiet_reference("mat", M.material_net(128), QGAMES)
    assert {r[5] for r in ref[3]} == {0, 1, 2, 3}                      # lines of every length at d = 3
    assert sum(r[3] for d in range(4) for r in ref[d]) < 20000         # the trees stay small
    assert sum(r[3] for r in ref[3]) > 1000
    plies = plies_of(QGAMES)
    trade = plies.index((Q.TRADE, ""))
    assert mref[2][trade] == (-1600, 0, -100, 2, 0, 0)                 # a stand-pat tie
    ep = plies.index((Q.EP[0], Q.EP[1]))
    assert ref[1][ep][3] == 1 and F.move_uci(F.game_captures(*Q.EP)[1][1]) == "e5d6"   # en passant in the tree
    promo = plies.index((Q.PROMO, ""))
    assert ref[1][promo][3] == 4                                       # a capturing promotion: four records
    first = plies.index((START, ""))
    assert all(ref[d][first][3] == 0 for d in range(4))                # a level without a capture


@pytest.mark.parametrize("net", ["rnd", "mat"])
def test_quiesce_matches_the_rule(data, ev, mat, net):
    e, bytes_ = (ev, data) if net == "rnd" else (mat, M.material_net(128))
    ref = quiet_reference(net, bytes_, QGAMES)
    woff = np.cumsum([0] + [len(mv.split()) + 1 for _, mv in QGAMES])
    for d in range(4):
        got, off = e.quiesce(QGAMES, d)
        assert off.tolist() == woff.tolist() and not got["reserved"].any()
        for p, (g, w) in enumerate(zip(Q.quiet_tuples(got), ref[d])):
            assert g == w, (d, p, plies_of(QGAMES)[p])
        assert len(got) == len(ref[d])
    # d = 0: the plies' own evaluation
    pos, _ = e.build_batch(QGAMES)
    ps, po = e.eval_positions(pos)
    got, _ = e.quiesce(QGAMES, 0)
    assert got["psqt"].tolist() == ps.tolist() and got["positional"].tolist() == po.tolist()
    assert not got["nodes"].any() and not got["len"].any() and not got["move"].any()
    # the depth exceeds the tree's height: it ends early
    for fen in (Q.BARE, Q.KQK, Q.HANGS):
        deep, _ = e.quiesce([(fen, "")], 4)
        three, _ = e.quiesce([(fen, "")], 3)
        assert deep.tobytes() == three.tobytes()


def test_quiesce_errors_and_capacity(ev):
    n, g = C.c_size_t(), C.c_size_t()
    text, fo, mo = F.pack_games([(START, "e2e4")])
    args = (text, len(text), N.ptr(fo), N.ptr(mo), 1)
    assert N.lib.fnnue_quiesce(ev._h, *args, 5, None, 0, None, 0, C.byref(n), C.byref(g)) == -1
    assert N.lib.fnnue_quiesce(ev._h, *args, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == -10
    assert (n.value, g.value) == (2, 1)
    assert N.lib.fnnue_set_search_quiesce(ev._h, 5) == -1 and N.lib.fnnue_set_search_quiesce(ev._h, -1) == -1
    assert ev.search_quiesce() == 0
    zh = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, 256, ZH), ZH), 0)
    try:
        assert N.lib.fnnue_quiesce(zh._h, *args, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == -4
    finally:
        zh.close()
    with pytest.raises(F.FnnueError) as err:
        ev.quiesce([(START, "e2e4"), (START, "e2e4 e2e4")], 1)
    assert err.value.code == -8 and "game 1" in str(err.value)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_a_frontier_of_63_64_65_expanding_nodes(ev, n):
    one, _ = ev.quiesce([TENSE], 3)
    assert int(one["nodes"][-1]) > 10
    got, off = ev.quiesce([(TENSE[0], TENSE[1])] * n, 3)
    assert len(got) == 3 * n and got.tobytes() == np.tile(one, n).tobytes()


def test_quiesce_does_not_depend_on_the_slices(ev):
    games = [TENSE] * 40 + QGAMES
    want, _ = ev.quiesce(games, 3)
    before = ev.quiesce_slices()
    ev.quiesce(games, 3)
    assert ev.quiesce_slices() - before == 1
    with env(FNNUE_QUIESCE_RECORDS=1):  # the floor: 256 records a level
        before = ev.quiesce_slices()
        got, _ = ev.quiesce(games, 3)
        assert ev.quiesce_slices() - before > 4
    assert got.tobytes() == want.tobytes()


# ---- 2. the searches against the reference with substituted terms ----

def ordered_lines1(ps, po, end, codes):
    """The depth-1 lines of one group, best first: R.reduce_group's key as a total order."""
    rows = []
    for c in range(1, len(ps)):
        one = R.reduce_group([ps[0], ps[c]], [po[0], po[c]], [end[0], end[c]], [0, codes[c]])
        rank = 2 if one[R.BEST["kind"]] == F.BEST_MATE else 1
        rows.append(((-rank, -one[R.BEST["value"]], c), (one[0], one[1], one[2], c, codes[c], one[R.BEST["kind"]], 0)))
    return [r for _, r in sorted(rows)]


@pytest.mark.parametrize("d", [1, 2])
def test_searches_match_the_reference_with_substituted_leaves(data, qe, d):
    ref = Q.search_reference(data, SGAMES, d)
    qe.set_search_quiesce(d)
    try:
        assert qe.search_quiesce() == d
        got = results(qe, SGAMES)
    finally:
        qe.set_search_quiesce(0)
    s1, s2 = as_tuples(got["s1"], F.BEST_DTYPE), as_tuples(got["s2"], F.BEST2_DTYPE)
    assert len(s1) == len(s2) == len(ref)
    kbt, kid = as_tuples(got["kb"], F.BEST_DTYPE), 0
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
    assert kid == len(kbt)


# ---- 3. invariants on the two-ply games, without a reference ----

@pytest.fixture(scope="module")
def plain(ev):
    return results(ev, R.GAMES)


def test_quiesce_zero_is_byte_identical(qe, plain):
    qe.set_search_quiesce(2)
    qe.set_search_quiesce(0)
    assert same(results(qe, R.GAMES), plain)


@pytest.mark.parametrize("d", [1, 2])
def test_invariants_with_the_setting_on(qe, plain, d):
    qe.set_search_quiesce(d)
    try:
        got = results(qe, R.GAMES)
        before = qe.quiesce_slices()
        with env(FNNUE_SEARCH2_RECORDS=1, FNNUE_QUIESCE_RECORDS=1):  # the smallest chunks and slices
            small = results(qe, R.GAMES)
        assert qe.quiesce_slices() - before > 20
    finally:
        qe.set_search_quiesce(0)
    assert same(small, got)
    assert not same(got, plain)                                     # the leaves did change
    for name in ("s1", "s2"):
        a, b = got[name], plain[name]
        assert a["nodes"].tolist() == b["nodes"].tolist() and a["end"].tolist() == b["end"].tolist()
        # the reported triple: value == trunc((psqt + positional) / 16) on every CP record whose value comes from an
        # evaluation (a stalemating move is worth 0 whatever its terms).  A two-move pv's terms are the depth-1
        # record's, from the child's side to move, as the second reduction has stored them since ABI 3.7: there
        # the value is the negated quotient.
        cp = (a["kind"] == F.BEST_CP) & (a["value"] != 0)
        s = a["psqt"].astype(np.int64) + a["positional"].astype(np.int64)
        quot = np.sign(s) * (np.abs(s) // 16)
        if name == "s2":
            quot = np.where(a["pv_len"] == 2, -quot, quot)
        assert cp.sum() > 30 and (a["value"][cp] == quot[cp]).all()
    assert got["kb"]["nodes"].tolist() == plain["kb"]["nodes"].tolist() and got["km"].tobytes() == plain["km"].tobytes()
    # slot 0 of the lines is the best record
    for best, lines, child in ((got["s1"], got["l1"], "best"), (got["s2"], got["l2"], "best")):
        first = lines[:, 0]
        has = best["kind"] != F.BEST_NONE
        for a, b in (("psqt", "psqt"), ("positional", "positional"), ("value", "value"), (child, "child"),
                     ("move", "move"), ("kind", "kind")):
            assert best[a][has].tolist() == first[b][has].tolist()


# ---- 4. behaviour on the material net ----

def test_one_ply_stops_hanging_the_queen(mat):
    try:
        off0, _ = mat.search1([(Q.HANGS, "")])
        mat.set_search_quiesce(1)
        on1, _ = mat.search1([(Q.HANGS, "")])
    finally:
        mat.set_search_quiesce(0)
    assert F.move_uci(int(off0["move"][0])) == "e2e5" and int(off0["value"][0]) == 800
    assert F.move_uci(int(on1["move"][0])) != "e2e5" and int(on1["value"][0]) == 700
    assert int(on1["nodes"][0]) == int(off0["nodes"][0])


def test_two_plies_the_reply_that_hangs_a_rook_flips_the_choice(mat):
    try:
        off0, _ = mat.search2([(Q.FLIP, "")])
        mat.set_search_quiesce(2)
        on2, _ = mat.search2([(Q.FLIP, "")])
    finally:
        mat.set_search_quiesce(0)
    assert (F.move_uci(int(off0["move"][0])), int(off0["value"][0])) == ("d4c2", -100)
    assert (F.move_uci(int(on2["move"][0])), int(on2["value"][0])) == ("a1b1", -100)
    assert int(on2["nodes"][0]) == int(off0["nodes"][0]) and int(on2["pv_len"][0]) == 2


# ---- 5. the draw rules beside it ----

@pytest.mark.parametrize("net", ["rnd", "mat"])
def test_drawn_leaves_stay_worth_zero(data, qe, mat, net):
    qe, data = (qe, data) if net == "rnd" else (mat, M.material_net(128))
    # test_gpu_draws' shuffle game, and the same shuffle behind 1. e4 d5, where exd5 and dxe4 are there to resolve
    games = [(D.START, " ".join([D.SHUFFLE] * 2)), (D.START, "e2e4 d7d5 " + " ".join([D.SHUFFLE] * 2))]
    W = 218

    def lines(draws, d):
        qe.set_search_draws(draws)
        qe.set_search_quiesce(d)
        try:
            best, _, ls = qe.search1_lines(games, W)
        finally:
            qe.set_search_draws(False)
            qe.set_search_quiesce(0)
        out = []
        for p in range(len(best)):
            rows = ls[p]
            out.append({int(r["child"]): (int(r["psqt"]), int(r["positional"]), int(r["value"]), int(r["kind"]))
                        for r in rows[rows["kind"] != F.BEST_NONE]})
        return out

    plain, drawn, quiet, both = lines(False, 0), lines(True, 0), lines(False, 2), lines(True, 2)
    ref = Q.search_reference(data, games, 2, two=False)
    marked = changed = 0
    prefixes = plies_of(games)
    for p in range(len(plain)):
        ps, po, end, codes = ref[p]["group"]
        assert set(plain[p]) == set(both[p]) == set(range(1, len(ps)))
        # the children that stand for the third time, from the host's history of the extended games
        ext = [(prefixes[p][0], (prefixes[p][1] + " " + t).strip()) for t in ref[p]["texts"]]
        hist, hoff = F.game_history(ext)
        third = [int(hist["seen"][hoff[i + 1] - 1]) >= 2 for i in range(len(ext))]
        for c in plain[p]:
            if third[c - 1]:                 # a drawn leaf: worth 0, and left alone by the quiescence
                marked += 1
                assert both[p][c] == drawn[p][c] and both[p][c][2] == 0
            else:                            # every other leaf follows the reference
                assert both[p][c] == quiet[p][c]
                assert both[p][c][:2] == (R.wrap_neg(ps[c]), R.wrap_neg(po[c])), (p, c)
                changed += both[p][c] != plain[p][c]
    # on the random net standing pat wins below these openings; on the material net dxe4 and exd5 are seen
    assert marked >= 2 and (changed >= 2 or net == "rnd")


# ---- 6. a variant context ----

def test_variant_context_accepts_and_ignores_the_setting():
    zh = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, 256, ZH), ZH), 0)
    try:
        games = [(ZH_START, "e2e4 d7d5 e4d5 d8d5")]
        a1, _ = zh.vsearch1(ZH, games)
        a2 = zh.vsearch2(ZH, games)[0]
        zh.set_search_quiesce(2)
        assert zh.search_quiesce() == 2
        b1, _ = zh.vsearch1(ZH, games)
        b2 = zh.vsearch2(ZH, games)[0]
        assert a1.tobytes() == b1.tobytes() and a2.tobytes() == b2.tobytes()
        with pytest.raises(F.FnnueError) as err:
            zh.search1(games)
        assert err.value.code == -4
    finally:
        zh.close()


# ---- 7. the actor ----

def test_actor_with_quiescence_matches_the_library(data, qe):
    made = [make_channel(data, quiesce=1, analysis_depth=1), make_channel(data, quiesce=1, analysis_plies=2),
            make_channel(data, analysis_depth=1), make_channel(data)]
    try:
        (q1, q2, d1, d0) = (stub for stub, _ in made)
        assert q1.quiesce() == 1 and d0.quiesce() == 0
        games = SGAMES + [SCANDI]
        bodies = bodies_of(games)
        qe.set_search_quiesce(1)
        try:
            best, goff = qe.search1(games)
            out, off = qe.search2(games)
        finally:
            qe.set_search_quiesce(0)
        zero = d0.go(bodies)
        for i, (rows, zrows) in enumerate(zip(q1.go(bodies), zero)):
            assert not isinstance(rows, B.PositionFailed), rows
            check_depth1(rows, zrows, best[goff[i]:goff[i + 1]])
        for i, (rows, zrows) in enumerate(zip(q2.go_pv(bodies), zero)):
            assert not isinstance(rows, B.PositionFailed), rows
            check_two_plies(rows, zrows, out[off[i]:off[i + 1]])
        assert strip(q1.go(bodies)) != strip(d1.go(bodies))     # the setting reaches the pieces
        # depth-0 analysis, move work and a crazyhouse batch in one call: as on a channel without the setting
        q1.set_analysis_depth(0)
        mixed = bodies_of(games[:3]) + bodies_of(games[3:5], work="move") + \
            [B.AcquireResponseBody("zh", ZH_START, "e2e4 d7d5 e4d5", variant="crazyhouse")]
        assert strip(q1.go(mixed)) == strip(d0.go(mixed))
    finally:
        for _, actor in made:
            actor.close()

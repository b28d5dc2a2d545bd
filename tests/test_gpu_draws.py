"""Repetition and fifty-move draws on the device (ABI 3.12), bit-exact: the
device history against the host's, the four reductions on hand-made end bytes
with FNNUE_END_DRAW against the rule in Python (tests/test_draws.py), the
searches with the rules on against the host-built reference field by field,
rules on over games without a draw and rules off over games with one equal to a
context that never heard of them, the independence of the marks from the chunk
cuts and from key collisions (fresh child processes), and the engine actor."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from tests import test_draws as D
from tests import test_search2 as R
from tests.conftest import ROOT, net_bytes
from tests.test_gpu_multipv2 import lines_of, make_channel, want_line
from tests.test_gpu_search2 import NORM, ZH, ZH_START, bodies_of, check_two_plies, strip, trunc_div

pytestmark = pytest.mark.gpu

DRAW_GAMES = D.DRAW_GAMES
MIN_RECORDS = 219 * 219
LONG = (D.START, " ".join([D.SHUFFLE] * 40))  # 161 plies, every one after the 8th with a third occurrence below it
K = 3
as_tuples = D.as_tuples


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
def on(data):
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    assert e.search_draws() is False
    e.set_search_draws(True)
    assert e.search_draws() is True
    yield e
    e.close()


def results(e, games):
    """Every search of `games` on one context -> {name: array}."""
    s1, off = e.search1(games)
    _, _, l1 = e.search1_lines(games, K)
    s2, _, kb, km = e.search2(games, children=True)
    s2b, _, l2 = e.search2_lines(games, K)
    assert s2b.tobytes() == s2.tobytes()
    return {"off": off, "s1": s1, "l1": l1, "s2": s2, "l2": l2, "kb": kb, "km": km}


@pytest.fixture(scope="module")
def searched(on, ev):
    """DRAW_GAMES with the rules on and off (computed once, never changed)."""
    return results(on, DRAW_GAMES), results(ev, DRAW_GAMES)


# ---- 1. the history ----

def test_device_history_equals_the_host(ev):
    games = D.HISTORY_GAMES + R.GAMES + [LONG]
    want, woff = F.game_history(games)
    got, off = ev.game_history(games)
    assert off.tolist() == woff.tolist() and got.tobytes() == want.tobytes()
    assert int(got["seen"].max()) == 40 and int(got["clock"].max()) == 65535


def test_device_history_device_form_and_capacity(ev):
    import ctypes as C
    import torch
    games = D.HISTORY_GAMES
    want, woff = F.game_history(games)
    dev = torch.device("cuda", 0)
    text, fen_off, mv_off = F.pack_games(games)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    ng, n = len(games), len(want)
    d_off = torch.full((ng + 1,), -1, dtype=torch.int32, device=dev)
    d_out = torch.full((n * 4,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    cn, cg = C.c_size_t(), C.c_size_t()
    args = (ev._h, C.c_void_p(d_text.data_ptr()), C.c_void_p(d_fo.data_ptr()), C.c_void_p(d_mo.data_ptr()), ng)
    for d, cap, o, ocap in ((None, 0, None, 0), (d_out.data_ptr(), n - 1, d_off.data_ptr(), ng + 1),
                            (d_out.data_ptr(), n, d_off.data_ptr(), ng)):
        rc = N.lib.fnnue_game_history_device(*args, C.c_void_p(d), cap, C.c_void_p(o), ocap, C.byref(cn), C.byref(cg), None)
        assert rc == -10 and (cn.value, cg.value) == (n, ng)
    torch.cuda.synchronize(dev)
    assert bool((d_out == 0xAB).all()) and bool((d_off == -1).all())
    assert ev.game_history_device(d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, d_out.data_ptr(), n,
                                  d_off.data_ptr(), ng + 1, None) == (n, ng)
    ev.check()
    assert d_out.cpu().numpy().tobytes() == want.tobytes() and d_off.cpu().numpy().tolist() == woff.tolist()
    with pytest.raises(F.FnnueError) as err:
        ev.game_history([(D.START, "e2e4"), (D.START, "e2e4 e2e4")])
    assert err.value.code == -8 and "game 1" in str(err.value)


# ---- 2. the reductions on hand-made end bytes ----

def hand_made():
    """Level-1 arrays and the children's records: groups of 1, 2, 5, 33 and 219 records with random end bytes
    (every combination of DRAW with NO_MOVES and CHECK), and the cases the rule names."""
    Dr, NM, CH = F.END_DRAW, F.END_NO_MOVES, F.END_CHECK
    rng = np.random.default_rng(11)
    ps, po, end, off, cb = [], [], [], [0], []

    def child(kind=F.BEST_CP, value=0, nodes=1, best=1, move=77, p=0, q=0):
        return (p, q, value if kind == F.BEST_CP else 0, nodes, best, move, kind, 0)

    def group(terms, flags, kids):
        assert len(terms) == len(flags) == len(kids) + 1
        ps.extend(t[0] for t in terms), po.extend(t[1] for t in terms), end.extend(flags), cb.extend(kids)
        off.append(len(end))

    bytes_ = [0, 0, 0, 0, 0, Dr, Dr, Dr | CH, NM, NM | CH, Dr | NM, Dr | NM | CH]
    for size in (1, 2, 5, 33, 219):
        terms = [(int(rng.integers(-2**31, 2**31)), int(rng.integers(-2**31, 2**31))) for _ in range(size)]
        terms = [t if rng.integers(0, 4) else (16 * int(rng.integers(-2, 3)), 0) for t in terms]  # ties around 0
        kids = [child(F.BEST_MATE if rng.integers(0, 8) == 0 else F.BEST_CP, int(rng.integers(-3, 4)) * int(rng.integers(0, 9000)),
                      int(rng.integers(1, 219)), int(rng.integers(1, 219)), int(rng.integers(1, 4096)),
                      int(rng.integers(-2**31, 2**31)), int(rng.integers(-2**31, 2**31))) for _ in range(size - 1)]
        flags = [0] + [int(rng.choice(bytes_)) for _ in range(size - 1)]
        if size == 219:
            flags = [0] + [f & ~NM if f & CH else f for f in flags[1:]]  # no mate: the values and the draws are ranked
        group(terms, flags, kids)
    z = (0, 0)
    group([z, z, z, (320, 0)], [0, 0, Dr, 0], [child(value=0), child(value=-50, p=3), child(value=20)])   # a draw ties a 0: the 0 first
    group([z, z, z, (320, 0)], [0, Dr, 0, 0], [child(value=-50, p=4, q=-2**31), child(value=0), child(value=20)])  # the draw first
    group([z, (160, 0), (-9, 1)], [0, 0, Dr | NM | CH], [child(value=-900), child(F.BEST_NONE, p=7)])     # stays a mate
    group([z, (160, 0), (-9, 1)], [0, 0, Dr], [child(value=5), child(F.BEST_MATE, nodes=30, p=2**31 - 1, q=-5)])  # b_c mates: worth 0
    group([z, (160, 0), (-9, 1)], [2, Dr | CH, Dr], [child(F.BEST_MATE), child(F.BEST_MATE)])             # every move draws
    n = len(end)
    moves = (np.arange(n) * 73 % 4096 + 64).astype(np.uint16)
    return (np.array(ps, dtype=np.int64).astype(np.int32), np.array(po, dtype=np.int64).astype(np.int32),
            np.array(end, dtype=np.uint8), moves, np.array(off, dtype=np.uint32), np.array(cb, dtype=F.BEST_DTYPE))


def padded(lines, k, width):
    return [lines[j] if j < len(lines) else (0,) * width for j in range(k)]


def test_reductions_honour_the_draw_bit(ev):
    ps, po, end, moves, off, cb = hand_made()
    cbt = as_tuples(cb, F.BEST_DTYPE)
    spans = [(int(o), int(e)) for o, e in zip(off[:-1], off[1:])]
    assert max(e - o for o, e in spans) == 219 and ((end & F.END_DRAW) != 0).sum() > 60
    for mv in (moves, None):
        sl = lambda a, o, e: None if a is None else a[o:e]
        want1 = [D.reduce_group(ps[o:e], po[o:e], end[o:e], sl(mv, o, e)) for o, e in spans]
        assert as_tuples(ev.best_children(ps, po, end, mv, off), F.BEST_DTYPE) == want1
        want2 = [D.reply_rule(end[o:e], sl(mv, o, e), cbt[o - g:e - g - 1]) for g, (o, e) in enumerate(spans)]
        assert as_tuples(ev.best_replies(end, mv, off, cb), F.BEST2_DTYPE) == want2
        for k in (1, 4, 218):
            lines, _ = ev.topk_children(ps, po, end, mv, off, k)
            want = [ln for o, e in spans for ln in padded(D.ordered_children(ps[o:e], po[o:e], end[o:e], sl(mv, o, e)), k, 7)]
            assert as_tuples(lines, F.LINE_DTYPE) == want, k
            lines, _ = ev.topk_replies(end, mv, off, cb, k)
            want = [ln for g, (o, e) in enumerate(spans)
                    for ln in padded(D.ordered_replies(end[o:e], sl(mv, o, e), cbt[o - g:e - g - 1]), k, 10)]
            assert as_tuples(lines, F.LINE2_DTYPE) == want, k
    rec1 = lambda g: dict(zip(F.BEST_DTYPE.names, want1[g]))
    rec2 = lambda g: dict(zip(F.BEST2_DTYPE.names, want2[g]))
    assert (rec1(5)["best"], rec1(5)["value"]) == (1, 0) and (rec1(6)["best"], rec1(6)["value"]) == (1, 0)
    assert (rec2(5)["best"], rec2(5)["pv_len"]) == (1, 2) and (rec2(6)["best"], rec2(6)["pv_len"], rec2(6)["psqt"]) == (1, 1, -4)
    assert rec2(6)["positional"] == -2**31                                          # negated with wrap-around
    assert rec1(7)["kind"] == F.BEST_MATE and (rec2(7)["kind"], rec2(7)["best"], rec2(7)["pv_len"]) == (F.BEST_MATE, 2, 1)
    assert (rec2(8)["best"], rec2(8)["value"], rec2(8)["kind"], rec2(8)["pv_len"], rec2(8)["nodes"]) == \
        (2, 0, F.BEST_CP, 1, 33)                                                     # 0 beats -5; its nodes counted
    assert (rec2(8)["psqt"], rec2(8)["positional"]) == (-(2**31 - 1), 5)
    assert (rec2(9)["kind"], rec2(9)["best"], rec2(9)["value"], rec2(9)["end"]) == (F.BEST_CP, 1, 0, 2)
    assert (rec1(9)["kind"], rec1(9)["best"], rec1(9)["value"], rec1(9)["psqt"]) == (F.BEST_CP, 1, 0, -160)


# ---- 3. the searches with the rules on ----

def test_searches_with_draws_against_the_reference(searched):
    got, plain = searched
    ref = D.reference()
    off = got["off"]
    assert off.tolist() == D.draw_offsets().tolist() == plain["off"].tolist()
    s1, s2 = as_tuples(got["s1"], F.BEST_DTYPE), as_tuples(got["s2"], F.BEST2_DTYPE)
    for i, (one, lines1, two, lines2, marked, marked2) in enumerate(ref):
        p = int(off[i + 1]) - 1
        assert s1[p] == one, (i, dict(zip(F.BEST_DTYPE.names, s1[p])), dict(zip(F.BEST_DTYPE.names, one)))
        assert as_tuples(got["l1"][p], F.LINE_DTYPE) == padded(lines1, K, 7), i
        assert s2[p] == two, (i, dict(zip(F.BEST2_DTYPE.names, s2[p])), dict(zip(F.BEST2_DTYPE.names, two)))
        assert as_tuples(got["l2"][p], F.LINE2_DTYPE) == padded(lines2, K, 10), i
        # the plies before the last: below ply 5 nothing is drawn; plies 5 and 6 of a longer cut are the last
        # plies of the shorter ones (the same history, so the same records)
        for q in range(p - int(off[i])):
            for name in ("s1", "l1", "s2", "l2"):
                same = plain[name][int(off[i]) + q] if q < 5 else got[name][int(off[q - 5 + 1]) - 1]
                assert got[name][int(off[i]) + q].tobytes() == same.tobytes(), (i, q, name)
    # nodes never change; the rules do change these answers
    assert got["s1"]["nodes"].tolist() == plain["s1"]["nodes"].tolist()
    assert got["s2"]["nodes"].tolist() == plain["s2"]["nodes"].tolist()
    last = lambda i: int(off[i + 1]) - 1
    assert got["l1"][last(D.I_CUT5)].tobytes() == plain["l1"][last(D.I_CUT5)].tobytes()
    assert got["s2"][last(D.I_CUT5)].tobytes() == plain["s2"][last(D.I_CUT5)].tobytes()
    for i in (D.I_K99, D.I_K98, D.I_K120):
        assert got["l2"][last(i)].tobytes() != plain["l2"][last(i)].tobytes(), i
    k99 = got["s2"][last(D.I_K99)]
    assert (int(k99["kind"]), F.move_uci(int(k99["move"])), int(k99["pv_len"])) == (F.BEST_MATE, "g6h6", 1)
    assert [int(v) for v in got["l1"][last(D.I_K99)]["value"][1:]] == [0, 0]


def test_drawn_children_carry_their_own_terms(on, ev, searched):
    """fnnue_search2_children: the drawn child f6g8 of ply 7 holds its own terms, every other field as searched
    (with the rules: below it g1f3 repeats for the third time)."""
    got, plain = searched
    p = int(got["off"][D.I_CUT7 + 1]) - 1
    km = got["km"].tolist()
    assert km == plain["km"].tolist()
    differ = [d for d in range(len(km)) if km[d][0] == p and got["kb"][d].tobytes() != plain["kb"][d].tobytes()]
    assert len(differ) == 1  # among ply 7's children only the drawn one
    d = differ[0]
    after = (D.START, " ".join(D.G1[:8]))  # the position after f6g8
    own, _ = on.search1([after])
    for name in ("value", "nodes", "best", "move", "kind", "end"):
        assert got["kb"][d][name] == own[-1][name]
    ps, po = ev.eval_positions(F.game_positions(*after)[-1:])
    assert (int(got["kb"][d]["psqt"]), int(got["kb"][d]["positional"])) == (int(ps[0]), int(po[0]))


def test_draws_on_marks_nothing_on_games_without_a_draw(on, ev):
    a, b = results(on, R.GAMES), results(ev, R.GAMES)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_draws_off_equals_a_context_never_set(on, ev, searched):
    _, plain = searched
    on.set_search_draws(False)
    try:
        back = results(on, DRAW_GAMES)
    finally:
        on.set_search_draws(True)
    for name in back:
        assert back[name].tobytes() == plain[name].tobytes(), name


def test_a_variant_context_accepts_and_ignores_the_setting():
    zh = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, 256, ZH), ZH), 0)
    try:
        games = [(ZH_START, F.random_vgame(1000, ZH, ZH_START, 12))]
        before = zh.vsearch2(ZH, games)[0].tobytes()
        zh.set_search_draws(True)
        assert zh.vsearch2(ZH, games)[0].tobytes() == before
    finally:
        zh.close()


# ---- 4. chunk cuts and key collisions: fresh child processes ----

CHILD = """
import sys
import numpy as np
import fishnet_amd as F
from tests.conftest import net_bytes
from tests import test_draws as D
from tests import test_search2 as R
from tests.test_gpu_draws import DRAW_GAMES, LONG, results
ev = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
ev.set_search_draws(True)
out = {"a_" + k: v for k, v in results(ev, DRAW_GAMES + [LONG]).items()}
out.update({"b_" + k: v for k, v in results(ev, R.GAMES).items()})
out["hist"], out["hoff"] = ev.game_history(D.HISTORY_GAMES + R.GAMES + [LONG])
np.savez(sys.argv[1], **out)
ev.close()
"""


@pytest.fixture(scope="module")
def in_process(on):
    out = {"a_" + k: v for k, v in results(on, DRAW_GAMES + [LONG]).items()}
    out.update({"b_" + k: v for k, v in results(on, R.GAMES).items()})
    out["hist"], out["hoff"] = on.game_history(D.HISTORY_GAMES + R.GAMES + [LONG])
    return out


@pytest.mark.parametrize("env", [{"FNNUE_SEARCH2_RECORDS": str(MIN_RECORDS)}, {"FNNUE_DRAW_KEY_BITS": "4"}],
                         ids=["chunks", "collisions"])
def test_results_do_not_depend_on_chunks_or_key_collisions(in_process, tmp_path, env):
    nodes = in_process["a_s2"]["nodes"].astype(np.int64)
    assert nodes.max() <= MIN_RECORDS and nodes.sum() > MIN_RECORDS and nodes.sum() < 16 << 20  # one chunk / several
    assert (in_process["hist"]["seen"] >= 2).sum() > 100  # down the long game every ply has a third occurrence below it
    path = str(tmp_path / "child.npz")
    subprocess.run([sys.executable, "-c", CHILD, path], cwd=ROOT, env=dict(os.environ, **env), check=True, timeout=300)
    child = np.load(path)
    assert sorted(child.files) == sorted(in_process)
    for name in child.files:
        assert child[name].tobytes() == in_process[name].tobytes(), name


# ---- 5. the engine actor ----

@pytest.fixture(scope="module")
def chans(data):
    """(2 plies with the draw rules, 2 plies without, never set), each with a crazyhouse net."""
    made = [make_channel(data, analysis_plies=2, draw_rules=True), make_channel(data, analysis_plies=2),
            make_channel(data)]
    yield tuple(stub for stub, _ in made)
    for _, actor in made:
        actor.close()


ACTOR_GAMES = [DRAW_GAMES[D.I_CUT7], DRAW_GAMES[D.I_K99], R.GAMES[0]]


def test_actor_with_draw_rules(chans, on, ev):
    dd, d2, d0 = chans
    assert dd.draw_rules() is True and d2.draw_rules() is False
    want = results(on, ACTOR_GAMES)
    off = want["off"]
    zh_body = [B.AcquireResponseBody("zh", ZH_START, F.random_vgame(1000, ZH, ZH_START, 20), variant="crazyhouse")]
    bodies = bodies_of(ACTOR_GAMES)
    res, zero = dd.go_pv(bodies + zh_body), d0.go(bodies)
    for i, (rows, zrows) in enumerate(zip(res[:-1], zero)):
        assert not isinstance(rows, B.PositionFailed), rows
        check_two_plies(rows, zrows, want["s2"][off[i]:off[i + 1]])
    # the drawn best move answers as a stalemating one: Cp(0), depth 1, a one-move pv
    k99 = res[1][0]
    assert (k99.score, k99.depth, k99.best_move, k99.reply) == (B.Score("mate", 1), 1, "g6h6", None)
    rec = want["s2"][off[1] - 1]
    last = res[0][-1]
    assert (last.best_move, last.depth, last.nodes) == (F.move_uci(int(rec["move"])), int(rec["pv_len"]), int(rec["nodes"]))
    part = json.loads(B.into_analysis(res[0]))[-1]
    assert part["pv"] == " ".join(m for m in (last.best_move, last.reply) if m) and part["depth"] == last.depth
    drawn_first = [(i, q) for i in (0, 1) for q, b in enumerate(want["s2"][off[i]:off[i + 1]])
                   if b["kind"] == F.BEST_CP and b["pv_len"] == 1 and b["value"] == 0]
    for i, q in drawn_first:
        r = res[i][q]
        assert (r.score, r.depth, r.reply) == (B.Score("cp", 0), 1, None)
        assert json.loads(B.into_analysis(res[i]))[q]["pv"] == r.best_move
    # the lines: f6g8 at ply 7 is a one-move line worth 0 wherever it ranks
    lres = dd.go_lines_pv(bodies_of(ACTOR_GAMES, multipv=K) + zh_body)
    got = lines_of(lres)
    for i in range(len(ACTOR_GAMES)):
        for q in range(int(off[i + 1] - off[i])):
            ls = want["l2"][off[i] + q]
            legal = int((ls["kind"] != F.BEST_NONE).sum())
            if legal:
                assert got[i][q] == [want_line(l, F.move_uci) for l in ls[:legal]], (i, q)
    k99_lines = got[1][0]
    assert k99_lines[0][:3] == ("mate", 1, ("g6h6",)) and all(l[:2] == ("cp", 0) and len(l[2]) == 1 for l in k99_lines[1:])
    # the crazyhouse batch: as on a channel without the setting; the ordinary batch: no stray mark
    assert strip([res[-1]]) == strip(d2.go_pv(zh_body)) and strip([lres[-1]]) == strip(d2.go_lines_pv(zh_body))
    assert strip([res[2]]) == strip(d2.go_pv(bodies[2:]))
    assert lines_of(lres[1:2]) != lines_of(d2.go_lines_pv(bodies_of(ACTOR_GAMES[1:2], multipv=K)))  # the rules matter
    # one ply: fnnue_search1's answers with the rules on
    dd.set_analysis_plies(1)
    try:
        one = dd.go(bodies)
        for i, rows in enumerate(one):
            for r, b in zip(rows, want["s1"][off[i]:off[i + 1]]):
                if b["kind"] == F.BEST_NONE:
                    continue
                score = B.Score("mate", 1) if b["kind"] == F.BEST_MATE else B.Score("cp", trunc_div(int(b["value"]) * 100, NORM))
                assert (r.score, r.depth, r.best_move, r.nodes) == (score, 1, F.move_uci(int(b["move"])), int(b["nodes"]))
    finally:
        dd.set_analysis_plies(2)
    # set back to off: a channel that was never set
    dd.set_draw_rules(False)
    try:
        assert dd.draw_rules() is False
        assert strip(dd.go_pv(bodies + zh_body)) == strip(d2.go_pv(bodies + zh_body))
        assert lines_of(dd.go_lines_pv(bodies_of(ACTOR_GAMES, multipv=K))) == \
            lines_of(d2.go_lines_pv(bodies_of(ACTOR_GAMES, multipv=K)))
    finally:
        dd.set_draw_rules(True)

"""The two-ply search on the device (ABI 3.7), bit-exact: the second reduction
on hand-made arrays against the rule in Python, fnnue_search2 against the
host-built reference of tests/test_search2.py (field by field, and every
child's own depth-1 record against fnnue_search1 on the extended game), the
independence of the results from the scratch budget and from the actor's piece
cuts (fresh child processes), the capacity protocol, and the engine actor at
two plies (score, depth, nodes, best move, reply, pv JSON) with 0 and 1 plies
left exactly as they were."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from tests import test_search2 as R
from tests.conftest import ROOT, net_bytes
from tests.positions import CHESS960, START

pytestmark = pytest.mark.gpu

GAMES = R.GAMES
NORM = 361
MIN_RECORDS = 219 * 219
ZH = N.VARIANT_CRAZYHOUSE
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
CROWDED = "rnbqkbnr/pppppppp/pppppppp/8/8/PPPPPPPP/PPPPPPPP/RNBQKBNR w - - 0 1"  # 48 pieces: replays, cannot be evaluated
# longer than one chunk at the smallest budget and than one piece at the smallest piece size
LONG_GAMES = GAMES + [(g["position"], " ".join(g["moves"].split()[:60])) for g in R.WCC[2:6]]


def as_tuples(recs, dtype):
    return [tuple(int(r[n]) for n in dtype.names) for r in recs]


@pytest.fixture(scope="module")
def data():
    return net_bytes(1, 256, 0)


@pytest.fixture(scope="module")
def ev(data):
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def searched(ev):
    """search2 of GAMES with the children's depth-1 records (computed once, never changed)."""
    out, off, kb, km = ev.search2(GAMES, children=True)
    for a in (out, off, kb, km):
        a.setflags(write=False)
    return out, off, kb, km


# ---- 1. the second reduction alone ----

def hand_made():
    """Groups of 0, 1, 2, 33, 64, 65 and 219 records, the special cases, a group cut by npos and one beyond it."""
    rng = np.random.default_rng(7)
    end, off, cb = [], [0], []

    def child(kind=F.BEST_CP, value=0, nodes=0, best=1, move=77, ps=0, po=0):
        return (ps, po, value if kind == F.BEST_CP else 0, nodes, best, move, kind, 0)

    def group(flags, kids):
        assert len(kids) == max(len(flags) - 1, 0)
        end.extend(flags), cb.extend(kids)
        off.append(len(end))

    for size in (0, 1, 2, 33, 64, 65, 219):
        kids = []
        for c in range(max(size - 1, 0)):
            kind = F.BEST_MATE if rng.integers(0, 10) == 0 else F.BEST_CP
            kids.append(child(kind, int(rng.integers(-30000, 30000)), int(rng.integers(1, 219)),
                              int(rng.integers(1, 219)), int(rng.integers(1, 4096)), int(rng.integers(-2**31, 2**31)),
                              int(rng.integers(-2**31, 2**31))))
        group([0] * size, kids)
    group([0] * 41, [child(value=-10, best=c + 1, nodes=3) for c in range(40)])           # level-1 tie: the lowest index
    group([2, 0, 0, 0], [child(value=5), child(value=-7, best=9, move=99, ps=11, po=-12), child(value=-7, best=2)])
    group([0, 0, 1, 0], [child(value=3), child(F.BEST_NONE, ps=40, po=-2**31), child(value=0)])  # stalemating move ties a 0: first
    group([0, 0, 0, 1], [child(value=3), child(value=0, ps=5), child(F.BEST_NONE, ps=6)])  # ... the other way round
    group([0, 0, 3, 3], [child(value=-900), child(F.BEST_NONE, ps=2**31 - 1, po=1), child(F.BEST_NONE)])  # two mates
    group([0, 0, 1, 0], [child(F.BEST_MATE), child(F.BEST_NONE, ps=-8), child(value=1)])   # a stalemate beats -1
    group([1, 0, 0, 0], [child(F.BEST_MATE, nodes=4, best=3, move=5), child(F.BEST_MATE, nodes=6), child(F.BEST_MATE)])  # mated
    group([0, 0, 0], [child(value=2**28), child(value=-2**28)])                            # the value's whole range
    group([0, 0, 0], [child(F.BEST_MATE), child(value=2**28)])                             # the worst value beats a mated
    group([0] * 71, [child(value=50)] * 69 + [child(value=-50, best=4)])                   # the maximum at the last record
    group([], [])
    group([3], [])                                                                         # a mated ply without children
    n = len(end)
    group([0, 0, 0, 0, 0], [child(value=1), child(value=-4), child(value=-9), child(value=-99)])  # cut to 3 records by npos
    group([0, 0], [child()])                                                               # wholly beyond npos
    npos = n + 3
    kept = len(cb) - 3
    return (np.array(end[:npos], dtype=np.uint8), (np.arange(npos) * 73 % 4096 + 64).astype(np.uint16),
            np.array(off, dtype=np.uint32), np.array(cb[:kept], dtype=F.BEST_DTYPE))


def rule_over_groups(end, moves, off, cb):
    out, base, npos = [], 0, len(end)
    cbt = as_tuples(cb, F.BEST_DTYPE)
    for o, e in zip(off[:-1], off[1:]):
        e = min(int(e), npos)
        o = min(int(o), e)
        nk = max(e - o - 1, 0)
        out.append(R.reply_rule(end[o:e], moves[o:e] if moves is not None else None, cbt[base:base + nk]))
        base += nk
    assert base == len(cbt)
    return out


def test_best_replies_on_hand_made_groups(ev):
    end, moves, off, cb = hand_made()
    assert int(off[-1]) > len(end)
    want = rule_over_groups(end, moves, off, cb)
    got = as_tuples(ev.best_replies(end, moves, off, cb), F.BEST2_DTYPE)
    assert got == want
    rec = lambda g: dict(zip(F.BEST2_DTYPE.names, got[g]))
    assert got[0] == (0,) * 12 and got[17] == (0,) * 12 and got[-1] == (0,) * 12
    assert rec(1)["kind"] == F.BEST_NONE and rec(1)["nodes"] == 0 and rec(1)["pv_len"] == 0
    assert rec(6)["nodes"] == 218 + int(cb["nodes"][160:378].sum())
    assert rec(7)["best"] == 1 and rec(7)["value"] == 10 and rec(7)["nodes"] == 40 + 120
    assert (rec(8)["best"], rec(8)["value"], rec(8)["reply_index"], rec(8)["reply"], rec(8)["psqt"], rec(8)["end"]) == \
        (2, 7, 9, 99, 11, 2)
    assert (rec(9)["best"], rec(9)["pv_len"], rec(9)["kind"], rec(9)["psqt"], rec(9)["positional"]) == \
        (2, 1, F.BEST_CP, -40, -2**31)                      # the child's own terms, negated with wrap-around
    assert (rec(10)["best"], rec(10)["pv_len"], rec(10)["psqt"]) == (2, 2, 5)
    assert (rec(11)["best"], rec(11)["kind"], rec(11)["pv_len"], rec(11)["psqt"], rec(11)["reply"]) == \
        (2, F.BEST_MATE, 1, -(2**31 - 1), 0)
    assert (rec(12)["best"], rec(12)["kind"], rec(12)["value"], rec(12)["pv_len"]) == (2, F.BEST_CP, 0, 1)
    assert (rec(13)["kind"], rec(13)["best"], rec(13)["reply_index"], rec(13)["reply"], rec(13)["nodes"], rec(13)["end"]) == \
        (F.BEST_MATED, 1, 3, 5, 13, 1)
    assert (rec(14)["best"], rec(14)["value"]) == (2, 2**28)
    assert (rec(15)["best"], rec(15)["value"], rec(15)["kind"]) == (2, -2**28, F.BEST_CP)
    assert (rec(16)["best"], rec(16)["value"], rec(16)["reply_index"]) == (70, 50, 4)
    assert got[18] == (0, 0, 0, 0, 0, 0, 0, 0, F.BEST_NONE, 3, 0, 0)
    assert (rec(19)["nodes"], rec(19)["best"], rec(19)["value"]) == (2, 2, 4)  # two of its four children are left
    # without a moves array: the same records, move 0
    bare = as_tuples(ev.best_replies(end, None, off, cb), F.BEST2_DTYPE)
    assert bare == rule_over_groups(end, None, off, cb) and all(r[6] == 0 for r in bare)


def test_best_replies_device_form_is_identical(ev):
    import torch
    end, moves, off, cb = hand_made()
    want = ev.best_replies(end, moves, off, cb)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev)
    d_end, d_moves, d_off, d_cb = up(end), up(moves), up(off), up(cb)
    d_out = torch.full((len(want) * N.BEST2_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ev.best_replies_device(d_end.data_ptr(), d_moves.data_ptr(), d_off.data_ptr(), len(off) - 1, len(end),
                           d_cb.data_ptr(), d_out.data_ptr(), None)
    ev.check()
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST2_DTYPE), want)


# ---- 2. search2 against the reference ----

def test_search2_matches_reference(searched):
    out, off, kb, km = searched
    ref, roff, per_child = R.reference()
    assert off.tolist() == roff.tolist()
    got = as_tuples(out, F.BEST2_DTYPE)
    for p, (g, w) in enumerate(zip(got, ref)):
        assert g == w, (p, dict(zip(F.BEST2_DTYPE.names, g)), dict(zip(F.BEST2_DTYPE.names, w)))
    assert len(got) == len(ref)
    assert {int(k) for k in out["kind"]} == {F.BEST_NONE, F.BEST_CP, F.BEST_MATE, F.BEST_MATED}
    # the children's own records, in record order with their (ply, child index)
    want_map = [(p, c + 1) for p, kids in enumerate(per_child) for c in range(len(kids))]
    assert [tuple(int(v) for v in m) for m in km] == want_map
    kbt = as_tuples(kb, F.BEST_DTYPE)
    d = 0
    for kids in per_child:
        for _, d1 in kids:
            if d1 is not None:
                assert kbt[d] == d1, d
            else:
                assert kbt[d][2:7] == (0, 0, 0, 0, F.BEST_NONE) and kbt[d][7] & F.END_NO_MOVES
            d += 1
    assert d == len(kbt)


def test_children_records_equal_search1_on_extended_games(ev, searched):
    _, _, kb, km = searched
    _, _, per_child = R.reference()
    prefixes = [(fen, mv.split()[:q]) for fen, mv in GAMES for q in range(len(mv.split()) + 1)]
    ext = [(prefixes[p][0], " ".join(prefixes[p][1] + [per_child[p][c - 1][0]])) for p, c in km.tolist()]
    best, goff = ev.search1(ext)
    last = best[goff[1:] - 1]
    has_move = last["kind"] != F.BEST_NONE
    assert has_move.sum() > 1000 and (~has_move).sum() >= 3
    assert np.array_equal(kb[has_move], last[has_move])
    for n in ("value", "nodes", "best", "move", "kind", "end"):  # a child without a legal move: its own terms instead of zeros
        assert np.array_equal(kb[n][~has_move], last[n][~has_move])


def test_search2_device_form_and_capacity_protocol(ev, searched):
    import ctypes as C
    import torch
    out, off, _, _ = searched
    dev = torch.device("cuda", 0)
    text, fen_off, mv_off = F.pack_games(GAMES)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    ng = len(GAMES)
    d_off = torch.full((ng + 1,), -1, dtype=torch.int32, device=dev)
    d_out = torch.full((len(out) * N.BEST2_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    n, g = C.c_size_t(), C.c_size_t()
    args = (ev._h, C.c_void_p(d_text.data_ptr()), C.c_void_p(d_fo.data_ptr()), C.c_void_p(d_mo.data_ptr()), ng)
    # sizing calls: the sizes come back, nothing is written
    for d, cap, o, ocap in ((None, 0, None, 0), (d_out.data_ptr(), len(out) - 1, d_off.data_ptr(), ng + 1),
                            (d_out.data_ptr(), len(out), d_off.data_ptr(), ng)):
        rc = N.lib.fnnue_search2_device(*args, C.c_void_p(d), cap, C.c_void_p(o), ocap, C.byref(n), C.byref(g), None)
        assert rc == -10 and (n.value, g.value) == (len(out), ng)
    torch.cuda.synchronize(dev)
    assert bool((d_out == 0xAB).all()) and bool((d_off == -1).all())
    assert ev.search2_device(d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, d_out.data_ptr(), len(out),
                             d_off.data_ptr(), ng + 1, None) == (len(out), ng)
    ev.check()
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST2_DTYPE), out)
    assert d_off.cpu().numpy().tolist() == off.tolist()
    assert np.array_equal(ev.search2(GAMES)[0], out)  # the plain host form


def test_search2_needs_a_chess_net_and_names_a_bad_move(ev):
    zh = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, 256, ZH), ZH), 0)
    try:
        with pytest.raises(F.FnnueError) as err:
            zh.search2([(START, "e2e4")])
        assert err.value.code == -4
    finally:
        zh.close()
    with pytest.raises(F.FnnueError) as err:
        ev.search2([(START, "e2e4"), (START, "e2e4 e2e4")])
    assert err.value.code == -8 and "game 1" in str(err.value)


# ---- 3. the scratch budget ----

BUDGET_CHILD = """
import sys
import numpy as np
import fishnet_amd as F
from tests.conftest import net_bytes
from tests.test_gpu_search2 import LONG_GAMES
ev = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
out, off = ev.search2(LONG_GAMES)
np.save(sys.argv[1], out)
ev.close()
"""


def test_results_do_not_depend_on_the_budget(ev, tmp_path):
    out, off = ev.search2(LONG_GAMES)
    # by the documented cuts (whole plies, at most the budget's records, a ply's records = its nodes) the smallest
    # budget walks these games in several chunks of some tens of plies; the default takes them in one
    nodes = out["nodes"].astype(np.int64)
    assert nodes.max() <= MIN_RECORDS and nodes.sum() < 16 << 20
    chunks, acc = 1, 0
    for x in nodes:
        if acc + x > MIN_RECORDS:
            chunks, acc = chunks + 1, 0
        acc += x
    assert chunks >= 4
    path = str(tmp_path / "small.npy")
    env = dict(os.environ, FNNUE_SEARCH2_RECORDS="1")  # forced up to one ply's maximum
    subprocess.run([sys.executable, "-c", BUDGET_CHILD, path], cwd=ROOT, env=env, check=True, timeout=300)
    small = np.load(path)
    assert small.dtype == F.BEST2_DTYPE and small.tobytes() == out.tobytes()


# ---- the engine actor ----

@pytest.fixture(scope="module")
def chans(data):
    """(a 2-plies channel, a set_analysis_depth(1) channel, a channel never set), each with a crazyhouse net."""
    zh = F.synthesize_variant_net(5, 256, ZH)
    made = []
    for kw in ({"analysis_plies": 2}, {"analysis_depth": 1}, {}):
        made.append(B.channel(F.Net.from_bytes(data), 0, crazyhouse=F.Net.from_bytes_variant(zh, ZH), **kw))
    yield tuple(stub for stub, _ in made)
    for _, actor in made:
        actor.close()


def bodies_of(games, **kw):
    return [B.AcquireResponseBody(f"g{i}", fen, mv, variant="chess960" if fen == CHESS960 else "fromPosition", **kw)
            for i, (fen, mv) in enumerate(games)]


def strip(res, reply=True):
    """Every field but time_ms / nps (and, on request, the reply)."""
    out = []
    for rows in res:
        if isinstance(rows, B.PositionFailed):
            out.append(("failed", rows.code))
        else:
            out.append([(r.position_id, r.skipped, r.score and (r.score.kind, r.score.value), r.psqt, r.positional,
                         r.depth, r.nodes, r.best_move, r.matrix, r.reply if reply else None) for r in rows])
    return out


def trunc_div(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)


def check_two_plies(rows, zero_rows, recs):
    assert len(rows) == len(recs)
    for q, (r, z, b) in enumerate(zip(rows, zero_rows, recs)):
        assert r.position_id == q
        if b["kind"] == F.BEST_NONE:  # exactly as on a never-set channel
            assert (z.depth, z.nodes, z.best_move) == (0, 0, None)
            assert (r.score, r.depth, r.nodes, r.best_move, r.reply, r.psqt, r.positional) == \
                (B.Score("mate" if b["end"] & F.END_CHECK else "cp", 0), 0, 0, None, None, z.psqt, z.positional)
            continue
        score = {F.BEST_MATE: B.Score("mate", 1), F.BEST_MATED: B.Score("mate", -1)}.get(
            int(b["kind"]), B.Score("cp", trunc_div(int(b["value"]) * 100, NORM)))
        assert (r.score, r.depth, r.nodes, r.best_move, r.reply, r.psqt, r.positional) == \
            (score, int(b["pv_len"]), int(b["nodes"]), F.move_uci(int(b["move"])),
             F.move_uci(int(b["reply"])) or None, int(b["psqt"]), int(b["positional"]))


def test_actor_two_plies_against_search2(chans, searched):
    d2, _, d0 = chans
    out, off, _, _ = searched
    bodies = bodies_of(GAMES)
    res, zero = d2.go_pv(bodies), d0.go(bodies)
    for i, (rows, zrows) in enumerate(zip(res, zero)):
        assert not isinstance(rows, B.PositionFailed), rows
        check_two_plies(rows, zrows, out[off[i]:off[i + 1]])
    assert B.last_stats(d2._actor)["positions"] == len(out) + int(out["nodes"].sum())  # plies + children + grandchildren
    assert strip(d2.go_pv(bodies)) == strip(res)  # the same call twice
    # go() and go_timeout(): the same responses without the reply
    plain = d2.go(bodies)
    assert all(r.reply is None for rows in plain for r in rows)
    assert strip(plain) == strip(res, reply=False)
    # the JSON: a mate in one is a one-move pv, elsewhere two moves, the mated ply, the finished game's last ply
    parts = json.loads(B.into_analysis(res[R.I_FINISHED]))
    assert parts[3]["pv"] == "d8h4" and parts[3]["score"] == {"mate": 1} and parts[3]["depth"] == 1
    assert len(parts[0]["pv"].split()) == 2 and parts[0]["depth"] == 2 and "cp" in parts[0]["score"]
    assert parts[0]["pv"] == res[R.I_FINISHED][0].best_move + " " + res[R.I_FINISHED][0].reply
    assert "pv" not in parts[4] and parts[4]["score"] == {"mate": 0} and parts[4]["depth"] == 0
    mated = json.loads(B.into_analysis(res[R.I_MATED]))[0]
    assert mated["score"] == {"mate": -1} and mated["pv"].endswith(" a2a1") and mated["depth"] == 2
    # the compact form: score and depth only
    compact = d2.go_compact(bodies_of(GAMES[4:], multipv=None))
    for rows, crows in zip(res[4:], compact):
        assert [(r.score, r.depth, r.psqt, r.positional) for r in rows] == \
            [(r.score, r.depth, r.psqt, r.positional) for r in crows]
        assert all(r.best_move is None for r in crows)


def test_actor_skipped_ids_are_kept(chans, searched):
    d2, _, _ = chans
    out, off, _, _ = searched
    fen, mv = GAMES[R.I_MATE1]
    rows = d2.go_pv([B.AcquireResponseBody("s", fen, mv, skip_positions=[1, 3])])[0]
    assert [r.skipped for r in rows] == [False, True, False, True]
    b = out[off[R.I_MATE1] + 2]
    assert (rows[2].best_move, rows[2].reply, rows[2].depth) == \
        (F.move_uci(int(b["move"])), F.move_uci(int(b["reply"])), 2)
    assert rows[1].reply is None and rows[3].reply is None


def test_actor_back_to_one_ply_and_zero(chans):
    d2, d1, d0 = chans
    bodies = bodies_of(GAMES) + [B.AcquireResponseBody("mv", START, "e2e4 e7e5", work="move")]
    zh_moves = F.random_vgame(1000, ZH, ZH_START, 30)
    zh_body = [B.AcquireResponseBody("zh", ZH_START, zh_moves, variant="crazyhouse")]
    try:
        # move work and a crazyhouse batch: the same at 0, 1 and 2 plies
        assert strip(d2.go_pv(bodies[-1:])) == strip(d1.go(bodies[-1:])) == strip(d0.go(bodies[-1:]))
        assert strip(d2.go_pv(zh_body)) == strip(d0.go(zh_body))
        lines2, lines1 = (d.go_lines(bodies_of(GAMES[5:], multipv=2)) for d in (d2, d1))  # MultiPV: a one-ply search
        assert strip(lines2) == strip(lines1) and lines2[0][0].depth == 1 and len(lines2[0][0].lines) == 2
        assert [[r.lines for r in rows] for rows in lines2] == [[r.lines for r in rows] for rows in lines1]
        d2.set_analysis_plies(0)
        assert strip(d2.go_pv(bodies)) == strip(d0.go(bodies))
        d2.set_analysis_plies(1)
        assert strip(d2.go_pv(bodies)) == strip(d1.go(bodies))
        for bad in (3, -1):
            with pytest.raises(F.FnnueError) as err:
                d2.set_analysis_plies(bad)
            assert err.value.code == -1
        with pytest.raises(F.FnnueError) as err:
            d2.set_analysis_depth(2)
        assert err.value.code == -1
        assert strip(d2.go_pv(bodies)) == strip(d1.go(bodies))  # a refused setter changes nothing
    finally:
        d2.set_analysis_plies(2)
    assert d2.go_pv(bodies[:1])[0][0].depth == 2


def test_actor_failures_stay_isolated(chans):
    d2, _, d0 = chans
    good = bodies_of(GAMES[:2])
    mixed = [good[0], B.AcquireResponseBody("bad", START, "e2e4 e7e5 e1e3"), good[1],
             B.AcquireResponseBody("crowded", CROWDED, "a3a4", variant="fromPosition")]
    res, alone = d2.go_pv(mixed), d2.go_pv(good)
    assert isinstance(res[1], B.PositionFailed) and res[1].code == -8
    assert isinstance(res[3], B.PositionFailed) and res[3].code == -6  # the evaluator rejects its positions
    assert strip([res[0], res[2]]) == strip(alone) and alone[0][0].depth == 2 and alone[0][0].reply


# ---- 8. the piece cuts ----

PIECES_CHILD = """
import json
import fishnet_amd as F
from fishnet_amd import backend as B
from tests.conftest import net_bytes
from tests.test_gpu_search2 import LONG_GAMES, bodies_of, strip
stub, actor = B.channel(F.Net.from_bytes(net_bytes(1, 256, 0)), 0, analysis_plies=2)
res = stub.go_pv(bodies_of(LONG_GAMES))
print("RESULT " + json.dumps({"rows": strip(res), "stats": B.last_stats(actor)}))
actor.close()
"""


def test_piece_cuts_do_not_change_the_answers(chans):
    d2, _, _ = chans
    res = d2.go_pv(bodies_of(LONG_GAMES))
    stats = B.last_stats(d2._actor)
    assert stats["pieces"] == 1
    env = dict(os.environ, FNNUE_BACKEND_PIECE_PLIES="1")  # forced up to its minimum: pieces of 16 plies
    out = subprocess.run([sys.executable, "-c", PIECES_CHILD], cwd=ROOT, env=env, check=True, capture_output=True,
                         text=True, timeout=300).stdout
    small = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert small["rows"] == json.loads(json.dumps(strip(res)))
    assert small["stats"]["pieces"] > 1
    plies = sum(len(rows) for rows in res)
    searched = sum(r.nodes for rows in res for r in rows)
    assert small["stats"]["positions"] == stats["positions"] == plies + searched

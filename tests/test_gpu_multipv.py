"""MultiPV at analysis depth 1 on the device (ABI 3.5), bit-exact: the top-k
reduction on hand-made arrays against a sort in Python (sizes at the lane-
stride, register-count and fast-path boundaries; ties, mates, stalemates, the
int32 extremes; ragged slots, clamped offsets, a canary behind lines_cap),
slot 0 against fnnue_best_children, fnnue_search1_lines against the oracle's
evaluation of the host builder's records ranked by that Python, and the engine
actor's go_lines (line counts, line 0, the lines themselves, the matrix JSON
with k rows; failure isolation; pieces cut between batches of different
multipv)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from oracle.oracle import OracleNet
from tests.conftest import ROOT, net_bytes
from tests.positions import CHESS960, START

pytestmark = pytest.mark.gpu

WCC = json.load(open(os.path.join(ROOT, "tests", "golden", "wcc_games.json")))["games"]
MANY = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"  # 218 legal moves
FOOLS_MATE = "f2f3 e7e5 g2g4 d8h4"
STALEMATE = ("7k/5Q2/5K2/8/8/8/8/8 w - - 0 1", "f6g6")
MATE_OR_STALEMATE = "7k/5Q2/5K2/8/8/8/8/8 w - - 0 1"  # Qg7 / Qf8 mate, Kg6 stalemates
C960_MOVES = F.random_game(15, CHESS960, 30)
NORM = 361

# the games of tests/test_gpu_search1.py (a copy: that module may move)
GAMES = [(g["position"], " ".join(g["moves"].split()[:40])) for g in WCC[:6]]
GAMES += [(CHESS960, C960_MOVES), (MANY, "")]
SEARCH_GAMES = GAMES + [(START, "f2f3 e7e5 g2g4"), (MATE_OR_STALEMATE, ""), (START, FOOLS_MATE), STALEMATE]

FILL = 0xA5  # what an unwritten slot's bytes read as


def wrap_neg(x):
    return ((-int(x) + 2**31) % 2**32) - 2**31


def trunc_div(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)


def ranked(ps, po, end, moves, o, e):
    """The children of the group [o, e) in fnnue_topk_children's order, as LINE_DTYPE tuples: a sort of
    (rank, value, -index), descending."""
    keys = []
    for c in range(1, e - o):
        f = int(end[o + c])
        if f & F.END_NO_MOVES:
            keys.append((2 if f & F.END_CHECK else 1, 0, -c))
        else:
            keys.append((1, -trunc_div(int(ps[o + c]) + int(po[o + c]), 16), -c))  # C truncation
    out = []
    for rank, value, c in sorted(keys, reverse=True):
        c = -c
        out.append((wrap_neg(ps[o + c]), wrap_neg(po[o + c]), value if rank == 1 else 0, c,
                    int(moves[o + c]) if moves is not None else 0, F.BEST_MATE if rank == 2 else F.BEST_CP, 0))
    return out


def topk_groups(ps, po, end, moves, off, line_off, cap=None):
    """fnnue_topk_children in Python: the slots array, FILL where nothing may be written."""
    npos = len(ps)
    cap = int(line_off[-1]) if cap is None else cap
    want = np.full(max(cap, 1) * N.LINE_BYTES, FILL, dtype=np.uint8).view(F.LINE_DTYPE)[:cap]
    for g in range(len(off) - 1):
        e = min(int(off[g + 1]), npos)
        o = min(int(off[g]), e)
        lo, hi = int(line_off[g]), int(line_off[g + 1])
        if e == o:
            continue
        order = ranked(ps, po, end, moves, o, e)
        for j in range(hi - lo):
            if lo + j < cap:
                want[lo + j] = order[j] if j < len(order) else (0,) * 7
    return want


def same(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


def arrays(ps, po, end, off):
    n = len(ps)
    return (np.array(ps, dtype=np.int64).astype(np.int32), np.array(po, dtype=np.int64).astype(np.int32),
            np.array(end, dtype=np.uint8), (np.arange(n) * 73 % 4096 + 64).astype(np.uint16),
            np.array(off, dtype=np.uint32))


@pytest.fixture(scope="module")
def data():
    return net_bytes(1, 256, 0)


@pytest.fixture(scope="module")
def ev(data):
    e = F.Evaluator(F.Net.from_bytes(data), 0)
    yield e
    e.close()


SIZES = (0, 1, 2, 32, 33, 34, 65, 219, 256, 257, 258, 600)  # records: 257 is the last fast-path group


def sized_groups():
    """Groups of SIZES records; values from a narrow range, so that ties occur, with a few mates and stalemates."""
    rng = np.random.default_rng(11)
    ps, po, end, off = [], [], [], [0]
    for size in SIZES:
        ps.extend(rng.integers(-400, 400, size) * 16)
        po.extend(rng.integers(-3, 3, size))
        flags = np.zeros(size, dtype=np.uint8)
        if size > 2:
            flags[rng.integers(1, size, max(1, size // 40))] = 3  # mates in one
            flags[rng.integers(1, size, max(1, size // 40))] = 1  # stalemates
        end.extend(flags)
        off.append(len(ps))
    return arrays(ps, po, end, off)


@pytest.mark.parametrize("k", [1, 3, 40, 218, 700])
def test_reduction_sizes(ev, k):
    ps, po, end, moves, off = sized_groups()
    got, line_off = ev.topk_children(ps, po, end, moves, off, k, fill=FILL)
    assert line_off.tolist() == [g * k for g in range(len(SIZES) + 1)]
    want = topk_groups(ps, po, end, moves, off, line_off)
    assert same(got, want)
    # the empty group's slots are untouched, a group of one record (no child) is all zero
    assert got[:k].tobytes() == bytes([FILL]) * (k * 20) and got[k:2 * k].tobytes() == bytes(k * 20)
    if k >= 599:
        g = got[11 * k: 12 * k]
        assert sorted(g["child"][:599].tolist()) == list(range(1, 600)) and not g[599:].tobytes().strip(b"\0")


def valued_groups():
    ps, po, end, off = [], [], [], [0]

    def group(p, q, f):
        ps.extend(p), po.extend(q), end.extend(f)
        off.append(len(ps))

    group([0] + [160] * 64, [0] + [-320] * 64, [0] * 65)                         # 64 equal children: index order
    group([0] + [16, 16, 32, 32, 32, 16, 48] * 6, [0] * 43, [0] * 43)            # runs of equal values
    group([0, 5, 7, 0, 0, 9, 0, 3], [0, 0, 0, 0, 0, 0, 0, 0], [0, 3, 0, 1, 0, 3, 1, 3])  # mates, stalemates, zeros
    group([0, 100, -100, 50, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 1])               # stalemates between + and -
    group([0, -2**31, 2**31 - 1, 0], [0, -2**31, 2**31 - 1, 0], [0] * 4)         # the int32 extremes, both in one sum
    group([0, 2**31 - 1, -2**31], [0, -2**31, 2**31 - 1], [0] * 3)               # and cancelling
    group([0] + list(range(-15, 16)), [0] * 32, [0] * 32)                        # sums in (-16, 16): all 0
    group([0, 15, -15, 16, -16, 17, -17, 31, -31, 32, -32], [0] * 11, [0] * 11)  # truncation toward zero
    group([0, 8, 8], [0, 8, 7], [0, 0, 0])                                       # 16 / 16 = 1, 15 / 16 = 0
    return arrays(ps, po, end, off)


def test_reduction_values(ev):
    ps, po, end, moves, off = valued_groups()
    counts = [int(e - o) for o, e in zip(off[:-1], off[1:])]
    line_off = np.cumsum([0] + counts).astype(np.uint32)  # a slot per record: one zero slot behind the children
    got, _ = ev.topk_children(ps, po, end, moves, off, line_off, fill=FILL)
    assert same(got, topk_groups(ps, po, end, moves, off, line_off))
    grp = lambda g: got[line_off[g]:line_off[g + 1]]
    assert grp(0)["child"].tolist() == list(range(1, 65)) + [0]
    g2 = grp(2)
    assert g2["child"].tolist() == [1, 5, 7, 2, 3, 4, 6, 0]  # the mates, then -7 / 16 = 0 and the zeros by index
    assert g2["kind"].tolist() == [F.BEST_MATE] * 3 + [F.BEST_CP] * 4 + [0] and g2["value"].tolist() == [0] * 8
    assert grp(3)["child"].tolist() == [2, 3, 4, 1, 0] and grp(3)["value"].tolist() == [6, 0, 0, -6, 0]
    g4 = grp(4)
    assert g4["child"].tolist() == [1, 3, 2, 0] and g4["value"].tolist() == [2**28, 0, -(2**28 - 1), 0]
    assert g4["psqt"].tolist() == [-2**31, 0, -2**31 + 1, 0]
    assert grp(5)["child"].tolist() == [1, 2, 0] and grp(5)["value"].tolist() == [0, 0, 0]
    assert grp(6)["child"].tolist() == list(range(1, 32)) + [0] and not grp(6)["value"].any()
    assert grp(7)["value"].tolist() == [2, 1, 1, 1, 0, 0, -1, -1, -1, -2, 0]
    assert grp(7)["child"].tolist() == [10, 4, 6, 8, 1, 2, 3, 5, 7, 9, 0]
    assert grp(8)["child"].tolist() == [2, 1, 0] and grp(8)["value"].tolist() == [0, -1, 0]


def test_reduction_slots_and_arguments(ev):
    ps, po, end, moves, off = sized_groups()
    ng = len(off) - 1
    sizes = [int(e - o) for o, e in zip(off[:-1], off[1:])]
    kids = [max(s - 1, 0) for s in sizes]
    # ragged within one call: 0, 1, 3, exactly the children, more than the children
    slots = [(0, 1, 3, kids[g], kids[g] + 5)[g % 5] for g in range(ng)]
    line_off = np.cumsum([0] + slots).astype(np.uint32)
    got, _ = ev.topk_children(ps, po, end, moves, off, line_off, fill=FILL)
    assert same(got, topk_groups(ps, po, end, moves, off, line_off))
    for k in (0, 1, 3):
        got, lo = ev.topk_children(ps, po, end, moves, off, k, fill=FILL)
        assert len(got) == k * ng and same(got, topk_groups(ps, po, end, moves, off, lo))
    # without a moves array: the same lines, move 0
    bare, _ = ev.topk_children(ps, po, end, None, off, line_off, fill=FILL)
    assert same(bare, topk_groups(ps, po, end, None, off, line_off)) and not bare["move"][bare["kind"] != FILL].any()
    # offsets beyond npos are clamped: the last groups lose their records
    npos = int(off[-3]) + 7
    cut = ev.topk_children(ps[:npos], po[:npos], end[:npos], moves[:npos], off, line_off, fill=FILL)[0]
    assert same(cut, topk_groups(ps[:npos], po[:npos], end[:npos], moves[:npos], off, line_off))
    assert (cut[line_off[-2]:]["kind"] == FILL).all()  # the last group is empty now: nothing written
    # the host form refuses a buffer smaller than the slots
    with pytest.raises(F.FnnueError) as err:
        ev.topk_children(ps, po, end, moves, off, line_off, lines_cap=int(line_off[-1]) - 1)
    assert err.value.code == -10


def test_device_form_never_writes_behind_lines_cap(ev):
    import torch
    ps, po, end, moves, off = sized_groups()
    ng = len(off) - 1
    line_off = (np.arange(ng + 1) * 40).astype(np.uint32)
    total = int(line_off[-1])
    dev = torch.device("cuda", 0)
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)
    d_ps, d_po, d_off, d_lo = up(ps, np.int32), up(po, np.int32), up(off, np.int32), up(line_off, np.int32)
    d_end, d_mv = up(end, np.uint8), up(moves, np.int16)
    for cap in (total, total - 1, 6 * 40 + 17, 40, 1, 0):  # cuts inside a group's children, its zero tail, at a group
        d_lines = torch.full((total * 20 + 64,), FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ev.topk_children_device(d_ps.data_ptr(), d_po.data_ptr(), d_end.data_ptr(), d_mv.data_ptr(), d_off.data_ptr(),
                                ng, len(ps), d_lo.data_ptr(), d_lines.data_ptr(), cap, None)
        torch.cuda.synchronize(dev)  # the kernel ran on the context's own stream
        raw = d_lines.cpu().numpy()
        assert raw[cap * 20:].tobytes() == bytes([FILL]) * (len(raw) - cap * 20), cap  # the canary
        assert same(raw[:cap * 20].view(F.LINE_DTYPE), topk_groups(ps, po, end, moves, off, line_off, cap)), cap


def test_slot0_equals_best_children(ev):
    for ps, po, end, moves, off in (sized_groups(), valued_groups()):
        best = ev.best_children(ps, po, end, moves, off)
        one, _ = ev.topk_children(ps, po, end, moves, off, 1)
        three, _ = ev.topk_children(ps, po, end, moves, off, 3)
        shared = ["psqt", "positional", "value", "move", "kind"]
        for lines in (one, three[0::3]):
            assert all(np.array_equal(lines[n], best[n]) for n in shared)
            assert np.array_equal(lines["child"], best["best"])
        assert (best["kind"] != F.BEST_NONE).sum() >= len(best) - 3


# ---- fnnue_search1_lines ----

@pytest.fixture(scope="module")
def wanted(ev, data):
    """What search1_lines of SEARCH_GAMES must give at k = 218: the oracle's evaluation of the host builder's
    records, ranked in Python with the host's end flags (computed once, never changed)."""
    pos, off, moves, end = ev.build_children(SEARCH_GAMES)
    first, g0 = [], 0
    for fen, mv in SEARCH_GAMES:
        hp, ho = F.game_children(fen, mv)  # the host builder's records
        n = len(ho) - 1
        assert np.array_equal(off[g0:g0 + n + 1] - off[g0], ho) and np.array_equal(pos[off[g0]:off[g0 + n]], hp)
        first.append(g0)
        g0 += n
    ops, opo, rc = OracleNet(data).eval_packed(pos, threads=8)
    assert rc == 0
    hend = np.array(end)
    for (fen, mv), f0 in list(zip(SEARCH_GAMES, first))[len(GAMES):]:  # the short games: the host's flags
        ms = mv.split()
        for q in range(len(ms) + 1):
            o, e = int(off[f0 + q]), int(off[f0 + q + 1])
            hend[o] = F.game_end(fen, ms[:q])
            for x in range(o + 1, e):
                hend[x] = F.game_end(fen, ms[:q] + [F.move_uci(int(moves[x]))])
    nply = len(off) - 1
    line_off = (np.arange(nply + 1) * 218).astype(np.uint32)
    lines = topk_groups(ops, opo, hend, moves, off, line_off).reshape(nply, 218)
    lines.setflags(write=False)
    return lines, first + [nply]


@pytest.fixture(scope="module")
def searched(ev):
    best, goff = ev.search1(SEARCH_GAMES)
    best.setflags(write=False)
    return best, goff


@pytest.mark.parametrize("k", [1, 3, 218])
def test_search1_lines_against_oracle(ev, wanted, searched, k):
    lines, goff = wanted
    best, off, got = ev.search1_lines(SEARCH_GAMES, k)
    assert off.tolist() == goff and got.shape == (len(lines), k)
    assert same(np.ascontiguousarray(got), np.ascontiguousarray(lines[:, :k]))
    assert same(best, searched[0]) and off.tolist() == searched[1].tolist()  # fnnue_search1's own output


def test_search1_lines_special_positions(ev, wanted):
    lines, goff = wanted
    def mates_first(slots, n):
        """The mating children lead, in index order; returns how many there are."""
        nm = int((slots["kind"] == F.BEST_MATE).sum())
        assert (slots["kind"][:nm] == F.BEST_MATE).all() and (slots["kind"][nm:n] == F.BEST_CP).all()
        assert (np.diff(slots["child"][:nm].astype(np.int64)) > 0).all() and not slots["value"][:nm].any()
        assert (np.diff(slots["value"][nm:n].astype(np.int64)) <= 0).all()
        return nm

    many = lines[goff[7]]
    assert (many["kind"] != F.BEST_NONE).all() and len({F.move_uci(int(m)) for m in many["move"]}) == 218
    assert sorted(many["child"].tolist()) == list(range(1, 219))
    assert mates_first(many, 218) == 7  # seven of the 218 moves mate: seven lines of mate 1, by index
    # Qg7 mates (Qf8+ is answered by Kh7, so it is the only mate), Kg6 stalemates: among the values, as 0
    both = lines[goff[9]]
    n = int((both["kind"] != F.BEST_NONE).sum())
    texts = [F.move_uci(int(m)) for m in both["move"][:n]]
    nm = mates_first(both, n)
    assert nm >= 1 and "f7g7" in texts[:nm] and set(texts[:nm]) <= {"f7g7", "f7f8"}
    at = texts.index("f6g6")
    assert at >= nm and both["value"][at] == 0 and both["kind"][at] == F.BEST_CP
    assert (both["value"][nm:at] >= 0).all() and (both["value"][at + 1:n] <= 0).all()
    assert not both[n:].tobytes().strip(b"\0") and 20 < n < 218
    assert not lines[goff[11] - 1].tobytes().strip(b"\0")  # fool's mate played out: no child, all slots zero


def test_search1_lines_device_form_and_capacity(ev, searched):
    import torch
    best, goff = searched
    _, _, want = ev.search1_lines(SEARCH_GAMES, 3)
    dev = torch.device("cuda", 0)
    text, fen_off, mv_off = F.pack_games(SEARCH_GAMES)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    ng, nply = len(SEARCH_GAMES), len(best)
    d_off = torch.zeros(ng + 1, dtype=torch.int32, device=dev)
    d_out = torch.zeros(nply * N.BEST_BYTES, dtype=torch.uint8, device=dev)
    d_lines = torch.full((nply * 3 * N.LINE_BYTES + 64,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    call = lambda lines_cap: ev.search1_lines_device(d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), ng, 3,
                                                     d_out.data_ptr(), nply, d_off.data_ptr(), ng + 1,
                                                     d_lines.data_ptr(), lines_cap, None)
    with pytest.raises(F.FnnueError) as err:  # one slot short: refused before any ply is expanded
        call(nply * 3 - 1)
    assert err.value.code == -10
    torch.cuda.synchronize(dev)
    assert d_lines.cpu().numpy().tobytes() == bytes([FILL]) * len(d_lines) and not d_out.cpu().numpy().any()
    assert call(nply * 3) == (nply, ng)
    ev.check()
    raw = d_lines.cpu().numpy()
    assert same(raw[:nply * 60].view(F.LINE_DTYPE).reshape(nply, 3), np.ascontiguousarray(want))
    assert raw[nply * 60:].tobytes() == bytes([FILL]) * 64
    assert np.array_equal(d_out.cpu().numpy().view(F.BEST_DTYPE), best) and d_off.cpu().numpy().tolist() == goff.tolist()
    # a variant net's context is refused
    zh = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, 256, N.VARIANT_CRAZYHOUSE),
                                              N.VARIANT_CRAZYHOUSE), 0)
    try:
        with pytest.raises(F.FnnueError) as err:
            zh.search1_lines([(START, "e2e4")], 3)
        assert err.value.code == -4
    finally:
        zh.close()


# ---- the engine actor ----

ZH = N.VARIANT_CRAZYHOUSE
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"


@pytest.fixture(scope="module")
def chans(data):
    """(a depth-1 channel, a channel never set), both with a crazyhouse net."""
    zh = F.synthesize_variant_net(5, 256, ZH)
    made = []
    for depth in (1, 0):
        kw = {"analysis_depth": 1} if depth else {}
        made.append(B.channel(F.Net.from_bytes(data), 0, crazyhouse=F.Net.from_bytes_variant(zh, ZH), **kw))
    yield made[0][0], made[1][0]
    for _, actor in made:
        actor.close()


def body(i, multipv, **kw):
    fen, mv = SEARCH_GAMES[i]
    return B.AcquireResponseBody(f"g{i}", fen, mv, variant="chess960" if fen == CHESS960 else "fromPosition",
                                 multipv=multipv, **kw)


def strip(res, with_lines=False):
    """Every field but time_ms / nps (and the lines, unless asked for)."""
    out = []
    for rows in res:
        if isinstance(rows, B.PositionFailed):
            out.append(("failed", rows.code))
        else:
            out.append([(r.position_id, r.skipped, r.score and (r.score.kind, r.score.value), r.psqt, r.positional,
                         r.depth, r.nodes, r.best_move, r.matrix) + ((r.lines,) if with_lines else ())
                        for r in rows])
    return out


def pv_lines(slots, count):
    return [B.PvLine(B.Score("mate", 1) if s["kind"] == F.BEST_MATE else
                     B.Score("cp", trunc_div(int(s["value"]) * 100, NORM)),
                     F.move_uci(int(s["move"])), int(s["psqt"]), int(s["positional"])) for s in slots[:count]]


def check_lines(rows, game, multipv, lines, goff, skipped=()):
    """The rows of a chess analysis batch over SEARCH_GAMES[game] against search1_lines' slots."""
    for q, r in enumerate(rows):
        slots = lines[goff[game] + q]
        nodes = int((slots["kind"] != F.BEST_NONE).sum())
        if q in skipped or not multipv or not nodes:
            assert r.lines is None, (game, q)
            continue
        assert r.nodes == nodes and len(r.lines) == min(multipv, nodes), (game, q)
        assert r.lines == pv_lines(slots, len(r.lines)), (game, q)
        top = r.lines[0]  # line 0 is the response itself
        assert (top.score, top.move, top.psqt, top.positional) == (r.score, r.best_move, r.psqt, r.positional)


def matrix_json(r):
    """A response as into_analysis must write it."""
    if r.skipped:
        return '{"skipped":true}'
    score = lambda s: {s.kind: s.value}
    tail = {"depth": r.depth, "nodes": r.nodes, "time": r.time_ms, **({"nps": r.nps} if r.nps else {})}
    nulls = [None] * r.depth
    if r.lines:
        part = {"pv": [nulls + [[l.move]] for l in r.lines], "score": [nulls + [score(l.score)] for l in r.lines]}
    elif r.matrix:
        part = {"pv": [nulls + [[r.best_move] if r.best_move else []]], "score": [nulls + [score(r.score)]]}
    else:
        part = {**({"pv": r.best_move} if r.best_move else {}), "score": score(r.score)}
    return json.dumps({**part, **tail}, separators=(",", ":"))


MIXED = [(0, None, {}), (1, 1, {}), (8, 3, {}), (7, 255, {}), (9, 255, {}), (2, 3, {"skip_positions": [0, 2, 40, 99]}),
         (10, 3, {}), (11, 3, {}), (6, 5, {})]  # game 10 ends in mate, game 11 in stalemate


def mixed_bodies():
    bodies = [body(i, mpv, **kw) for i, mpv, kw in MIXED]
    bodies.insert(3, B.AcquireResponseBody("mv", START, "e2e4 e7e5", work="move"))
    bodies.insert(6, B.AcquireResponseBody("zh", ZH_START, F.random_vgame(1000, ZH, ZH_START, 12), variant="crazyhouse",
                                           multipv=3))
    return bodies


def test_actor_go_lines(chans, wanted):
    d1, _ = chans
    lines, goff = wanted
    bodies = mixed_bodies()
    assert B.lines_bound(bodies) == sum((len(b.moves.split()) + 1) * min(b.multipv, 218) for b in bodies
                                        if b.multipv and b.work == "analysis")
    res = d1.go_lines(bodies)
    assert not [r for r in res if isinstance(r, B.PositionFailed)]
    assert strip(res) == strip(d1.go(bodies))  # the responses are go()'s
    chess = [b for b in bodies if b.batch_id not in ("mv", "zh")]
    for (game, mpv, kw), b in zip(MIXED, chess):
        rows = res[bodies.index(b)]
        assert len(rows) == goff[game + 1] - goff[game]
        check_lines(rows, game, mpv, lines, goff, kw.get("skip_positions", ()))
    assert all(r.lines is None for i in (3, 6) for r in res[i])  # move work, the crazyhouse batch
    assert res[6][0].depth == 0 and res[6][0].matrix
    assert len(res[4][0].lines) == 218 and len(res[2][3].lines) == 3 and len(res[1][0].lines) == 1
    assert [l.score.kind for l in res[4][0].lines[:8]] == ["mate"] * 7 + ["cp"]  # the 218-move position's mates
    assert res[5][0].lines[0] == B.PvLine(B.Score("mate", 1), "f7g7", res[5][0].psqt, res[5][0].positional)
    assert B.PvLine(B.Score("cp", 0), "f6g6", *[(l.psqt, l.positional) for l in res[5][0].lines
                                                 if l.move == "f6g6"][0]) in res[5][0].lines  # the stalemate: cp 0
    assert res[8][-1].lines is None and res[8][-1].score == B.Score("mate", 0)   # the game that ends in mate
    assert res[9][-1].lines is None and res[9][-1].score == B.Score("cp", 0)     # and in stalemate
    assert strip(d1.go_lines(bodies), True) == strip(res, True)  # the same call twice
    for i in (2, 5, 7, 8, 9):
        assert B.into_analysis(res[i]) == "[" + ",".join(matrix_json(r) for r in res[i]) + "]"
    first = json.loads(B.into_analysis(res[2]))[3]
    assert first["pv"][0] == [None, ["d8h4"]] and first["score"][0] == [None, {"mate": 1}] and len(first["pv"]) == 3


def test_actor_depth0_has_no_lines(chans):
    d1, d0 = chans
    bodies = mixed_bodies()
    res = d0.go_lines(bodies)
    assert all(r.lines is None for rows in res for r in rows) and strip(res) == strip(d0.go(bodies))
    try:
        d1.set_analysis_depth(0)
        back = d1.go_lines(bodies)
    finally:
        d1.set_analysis_depth(1)
    assert strip(back, True) == strip(res, True)


def test_actor_failure_isolation_and_capacity(data):
    stub, actor = B.channel(F.Net.from_bytes(data), 0, analysis_depth=1)
    try:
        good = [body(8, 3), body(9, 3)]
        mixed = [good[0], B.AcquireResponseBody("bad", START, "e2e4 e7e5 e1e3", multipv=3), good[1]]
        res, alone = stub.go_lines(mixed), stub.go_lines(good)
        assert isinstance(res[1], B.PositionFailed) and res[1].code == -8
        assert strip([res[0], res[2]], True) == strip(alone, True) and len(alone[0][0].lines) == 3
        assert B.last_stats(actor)["pieces"] == 1
        # the raw call: the failed batch's range of lines is empty
        a, _keep = B._acquired(mixed)
        cap, bound = 4 + 4 + 1, B.lines_bound(mixed)
        assert bound == 27
        out = (B._Response * cap)()
        pv = (B._PvLine * bound)()
        off, loff = np.zeros(4, dtype=np.uint32), np.zeros(cap + 1, dtype=np.uint32)
        rc = np.zeros(3, dtype=np.int32)
        N.check(N.lib.fnnue_backend_go_lines(actor._h, a, 3, out, cap, N.ptr(off), N.ptr(rc), pv, bound, N.ptr(loff), 0))
        assert rc.tolist() == [0, -8, 0] and off.tolist() == [0, 4, 8, 9]
        assert loff[4] == loff[8] == 12 and (np.diff(loff.astype(np.int64)) >= 0).all()
        assert loff.tolist()[:5] == [0, 3, 6, 9, 12] and loff[9] == 15
        # one line short of the bound: refused before any work
        assert N.lib.fnnue_backend_go_lines(actor._h, a, 3, out, cap, N.ptr(off), N.ptr(rc), pv, bound - 1, N.ptr(loff),
                                            0) == -10
        with pytest.raises(F.FnnueError) as err:
            stub.go_lines(mixed, lines_cap=bound - 1)
        assert err.value.code == -10
    finally:
        actor.close()


CHILD = """
import json, sys
import fishnet_amd as F
from fishnet_amd import backend as B
from tests.conftest import net_bytes
from tests import test_gpu_multipv as T
stub, actor = B.channel(F.Net.from_bytes(net_bytes(1, 256, 0)), 0, analysis_depth=1)
res = stub.go_lines(T.straddling_bodies())
print("pieces", B.last_stats(actor)["pieces"])
print("result", json.dumps(T.strip(res, True), default=lambda o: o.__dict__))
actor.close()
"""


def straddling_bodies():
    return [body(i % 9, (None, 1, 3, 5, 255)[(i // 2) % 5]) for i in range(54)]


def test_actor_pieces_cut_between_different_multipv(chans):
    """FNNUE_BACKEND_PIECE_PLIES is read when the channel is made: a child process with pieces of 1024 plies."""
    d1, _ = chans
    env = dict(os.environ, FNNUE_BACKEND_PIECE_PLIES="1024")
    out = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, check=True, capture_output=True,
                         text=True, timeout=120).stdout
    pieces = int([ln for ln in out.splitlines() if ln.startswith("pieces ")][-1].split()[1])
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("result ")][-1][7:])
    assert pieces >= 2
    want = d1.go_lines(straddling_bodies())
    assert B.last_stats(d1._actor)["pieces"] == 1
    assert got == json.loads(json.dumps(strip(want, True), default=lambda o: o.__dict__))

"""MultiPV at two plies on the device (ABI 3.11), bit-exact: the ranking kernel
alone on hand-made arrays against the total order in Python
(tests/test_multipv2.py), fnnue_search2_lines against the host-built reference
of tests/test_search2.py and against the order applied to the search's own
child records, fnnue_vsearch2_lines on the variants' games (a crazyhouse ply
beyond the 256-child fast path included), the independence of the lines from
the scratch budget and the actor's piece cuts (fresh child processes), the
capacity protocol, and the engine actor's go_lines_pv at 2, 1 and 0 plies."""
import ctypes as C
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
from tests import test_multipv2 as M
from tests import test_search2 as R
from tests import test_vsearch2 as V
from tests.conftest import ROOT, net_bytes
from tests.positions import CHESS960, START

pytestmark = pytest.mark.gpu

GAMES = R.GAMES
NORM = 361
ZH, AT, KOTH = N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL
LINE2 = F.LINE2_DTYPE
FILL = 0xAB


def as_tuples(recs):
    return [tuple(int(r[n]) for n in recs.dtype.names) for r in recs]


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
    """search2 of GAMES with the children's records, and the level-1 arrays (computed once, never changed)."""
    out, off, kb, km = ev.search2(GAMES, children=True)
    _, coff, moves, end = ev.build_children(GAMES)
    for a in (out, off, kb, km, coff, moves, end):
        a.setflags(write=False)
    return out, off, kb, km, coff, moves, end


# ---- 1. the kernel alone ----

def hand_made(variant):
    """The hand-made arrays of the second reduction's tests (groups of 0, 1, 2, 33, 64, 65, 219 records, the
    variants' also 307; every special case; an empty group between others; a group cut by npos and one beyond
    it) behind groups of 257, 258 and 300 records: both sides of the 256-child fast path."""
    if variant:
        from tests.test_gpu_vsearch2 import hand_made as base
        flags = [0, 0, 0, F.END_CHECK, F.END_NO_MOVES, F.END_NO_MOVES | F.END_EXTINCT, F.END_WON,
                 F.END_WON | F.END_NO_MOVES | F.END_VARIANT]
        kinds = [F.BEST_CP] * 6 + [F.BEST_MATE, F.BEST_LOST]
    else:
        from tests.test_gpu_search2 import hand_made as base
        flags = [0, 0, 0, 0, 0, 1, 2, 3]
        kinds = [F.BEST_CP] * 7 + [F.BEST_MATE]
    rng = np.random.default_rng(23)
    end, off, cb = [], [0], []
    for size in (257, 258, 300):
        end.append(0)
        for _ in range(size - 1):
            f = int(flags[rng.integers(0, len(flags))])
            kind = F.BEST_NONE if f & F.END_NO_MOVES else int(kinds[rng.integers(0, len(kinds))])
            end.append(f)
            # few distinct values: ties at every place of the order, not only at its head
            cb.append(V.kid(kind, int(rng.integers(-40, 40)), int(rng.integers(0, 400)), int(rng.integers(1, 300)),
                            int(rng.integers(1, 4096)), int(rng.integers(-2**31, 2**31)),
                            int(rng.integers(-2**31, 2**31))))
        off.append(len(end))
    b_end, _, b_off, b_cb = base()
    shift = len(end)
    end = np.concatenate([np.array(end, dtype=np.uint8), b_end])
    off = np.concatenate([np.array(off, dtype=np.uint32), b_off[1:] + np.uint32(shift)])
    cb = np.concatenate([np.array(cb, dtype=F.BEST_DTYPE), b_cb])
    moves = (np.arange(len(end)) * 73 % 4096 + 64).astype(np.uint16)
    assert int(off[-1]) > len(end)  # the last groups are cut by npos
    return end, moves, off, cb


def children_counts(end, off):
    npos = len(end)
    e = np.minimum(off[1:].astype(np.int64), npos)
    o = np.minimum(off[:-1].astype(np.int64), e)
    return np.maximum(e - o - 1, 0), e - o


def slot_offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


@pytest.mark.parametrize("variant", [False, True], ids=["chess", "variant"])
def test_topk_replies_on_hand_made_groups(ev, variant):
    end, moves, off, cb = hand_made(variant)
    cbt = as_tuples(cb)
    nkid, nrec = children_counts(end, off)
    assert {257 - 1, 258 - 1, 300 - 1, 0, 1, 32, 63, 64, 218} <= set(nkid.tolist()) and 0 in nrec.tolist()
    topk = ev.vtopk_replies if variant else ev.topk_replies
    reduce2 = ev.vbest_replies if variant else ev.best_replies
    # slot counts 0, 1, 3, exactly the children, children + 5 and 218, walked over the groups so that the large
    # groups (the first three) get 1, 3 and exactly their children, and the later ones every count
    pattern = [lambda n: 1, lambda n: 3, lambda n: n, lambda n: n + 5, lambda n: 218, lambda n: 0]
    mixed = slot_offsets([pattern[g % 6](int(n)) for g, n in enumerate(nkid)])
    plus5 = slot_offsets([int(n) + 5 for n in nkid])
    best2 = as_tuples(reduce2(end, moves, off, cb))
    for line_off in (mixed, plus5, slot_offsets([3] * len(nkid)), slot_offsets([218] * len(nkid))):
        got, _ = topk(end, moves, off, cb, line_off, fill=FILL)
        want = M.lines_over_groups(end, moves, off, cbt, line_off, variant, fill=FILL)
        bad = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
        assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
        # slot 0 is the second reduction's record on every shared field, for every group with a slot
        for g in range(len(nkid)):
            if nrec[g] and line_off[g + 1] > line_off[g]:
                assert M.shared_of_line(as_tuples(got[line_off[g]:line_off[g] + 1])[0]) == M.shared_of_best2(best2[g]), g
    # slots >= children: the children are a permutation of 1..n, the five slots behind them all-zero
    got, _ = topk(end, moves, off, cb, plus5, fill=FILL)
    for g, n in enumerate(nkid):
        grp = got[plus5[g]:plus5[g + 1]]
        if nrec[g] == 0:
            assert grp.tobytes() == bytes([FILL]) * (5 * N.LINE2_BYTES)  # an empty group writes nothing
            continue
        assert sorted(grp["child"][:n].tolist()) == list(range(1, n + 1))
        assert grp[n:].tobytes() == bytes(5 * N.LINE2_BYTES) and (grp["kind"][:n] != F.BEST_NONE).all()
    # every class of the order is there
    kinds = {(int(k), int(p)) for k, p in zip(got["kind"], got["pv_len"])}
    want_kinds = {(F.BEST_MATE, 1), (F.BEST_CP, 1), (F.BEST_CP, 2), (F.BEST_MATED, 2)}
    if variant:
        want_kinds |= {(F.BEST_LOST, 1), (F.BEST_MATE, 2)}
    assert want_kinds <= kinds
    # without a moves array: the same lines, move 0 (the reply stays: it comes from the child's record)
    bare, _ = topk(end, None, off, cb, mixed, fill=FILL)
    assert bare.tobytes() == M.lines_over_groups(end, None, off, cbt, mixed, variant, fill=FILL).tobytes()
    # the host form refuses a buffer below line_off[-1]
    with pytest.raises(F.FnnueError) as err:
        topk(end, moves, off, cb, mixed, lines_cap=int(mixed[-1]) - 1)
    assert err.value.code == -10


@pytest.mark.parametrize("variant", [False, True], ids=["chess", "variant"])
def test_topk_replies_device_form_stops_at_lines_cap(ev, variant):
    import torch
    end, moves, off, cb = hand_made(variant)
    nkid, _ = children_counts(end, off)
    line_off = slot_offsets([int(n) + 5 for n in nkid])
    total = int(line_off[-1])
    # the capacity ends inside the second group's children; behind it a guard region of the same buffer
    cap = int(line_off[1]) + 100
    assert line_off[1] < cap < line_off[2] - 5
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev)
    d_end, d_moves, d_off, d_cb, d_loff = up(end), up(moves), up(off), up(cb), up(line_off)
    d_lines = torch.full((total * N.LINE2_BYTES,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    fn = ev.vtopk_replies_device if variant else ev.topk_replies_device
    fn(d_end.data_ptr(), d_moves.data_ptr(), d_off.data_ptr(), len(off) - 1, len(end), d_cb.data_ptr(),
       d_loff.data_ptr(), d_lines.data_ptr(), cap, None)
    ev.check()
    got = d_lines.cpu().numpy().view(LINE2)
    want = M.lines_over_groups(end, moves, off, as_tuples(cb), line_off, variant, cap=cap, fill=FILL)
    assert got[:cap].tobytes() == want.tobytes()
    assert got[cap:].tobytes() == bytes([FILL]) * ((total - cap) * N.LINE2_BYTES)  # the guard is untouched
    # the whole buffer: the host form's bytes
    d_lines.fill_(FILL)
    torch.cuda.synchronize(dev)
    fn(d_end.data_ptr(), d_moves.data_ptr(), d_off.data_ptr(), len(off) - 1, len(end), d_cb.data_ptr(),
       d_loff.data_ptr(), d_lines.data_ptr(), total, None)
    ev.check()
    host, _ = (ev.vtopk_replies if variant else ev.topk_replies)(end, moves, off, cb, line_off, fill=FILL)
    assert d_lines.cpu().numpy().tobytes() == host.tobytes()


def test_vtopk_replies_equals_topk_replies_on_chess_inputs(ev):
    end, moves, off, cb = hand_made(False)
    nkid, _ = children_counts(end, off)
    line_off = slot_offsets([int(n) + 5 for n in nkid])
    a, _ = ev.topk_replies(end, moves, off, cb, line_off, fill=FILL)
    b, _ = ev.vtopk_replies(end, moves, off, cb, line_off, fill=FILL)
    assert a.tobytes() == b.tobytes()


# ---- 2. search2_lines against the reference ----

def reference_lines(data):
    """Per ply of GAMES, every line in order, from the host reference of tests/test_search2.py: its children's
    depth-1 tuples, and for a child without a legal move its end flags and own terms from the host and the oracle."""
    ref, off, per_child = R.reference()
    prefixes = [(fen, mv.split()[:q]) for fen, mv in GAMES for q in range(len(mv.split()) + 1)]
    ended = [(p, c) for p, kids in enumerate(per_child) for c, (_, d1) in enumerate(kids) if d1 is None]
    recs = np.array([F.game_positions(prefixes[p][0], prefixes[p][1] + [per_child[p][c][0]])[-1] for p, c in ended],
                    dtype=np.uint8).reshape(-1, 36)
    ps, po, rc = OracleNet(data).eval_packed(recs, threads=4)
    assert rc == 0 and len(ended) >= 3
    own = {pc: (int(ps[i]), int(po[i])) for i, pc in enumerate(ended)}
    out = []
    for p, kids in enumerate(per_child):
        fen, prefix = prefixes[p]
        end, cb = [ref[p][R.B2["end"]]], []
        for c, (text, d1) in enumerate(kids):
            if d1 is None:
                f = F.game_end(fen, prefix + [text])
                end.append(f)
                cb.append(own[(p, c)] + (0, 0, 0, 0, F.BEST_NONE, f))
            else:
                end.append(0)
                cb.append(d1)
        out.append(M.ordered_lines(end, [0] + [R.code_of(t) for t, _ in kids], cb, False))
    return out, off


def padded(lines, k):
    return (lines + [(0,) * 10] * k)[:k]


@pytest.fixture(scope="module")
def lines218(ev):
    out, off, lines = ev.search2_lines(GAMES, 218)
    for a in (out, off, lines):
        a.setflags(write=False)
    return out, off, lines


def test_search2_lines_matches_reference(ev, data, searched, lines218):
    out, off, kb, km, coff, moves, end = searched
    ref_lines, roff = reference_lines(data)
    cbt = as_tuples(kb)
    for k in (1, 3, 218):
        got_out, got_off, lines = lines218 if k == 218 else ev.search2_lines(GAMES, k)
        assert got_out.tobytes() == out.tobytes() and got_off.tobytes() == off.tobytes()  # search2's bytes
        assert got_off.tolist() == roff.tolist() and lines.shape == (len(out), k)
        for p in range(len(out)):
            assert as_tuples(lines[p]) == padded(ref_lines[p], k), (k, p)
        # ... and the order applied to the search's own child records
        want = M.lines_over_groups(end, moves, coff, cbt, slot_offsets([k] * len(out)), False)
        assert lines.reshape(-1).tobytes() == want.tobytes()
        # slot 0 is the ply's record
        b2 = as_tuples(out)
        for p in range(len(out)):
            assert M.shared_of_line(as_tuples(lines[p][:1])[0]) == M.shared_of_best2(b2[p]), p


def test_search2_lines_special_plies(lines218):
    out, off, lines = lines218
    text = lambda l: (F.move_uci(int(l["move"])), F.move_uci(int(l["reply"])))
    live = lambda p: lines[p][lines[p]["kind"] != F.BEST_NONE]
    # a mate in one is there: line 0 is d8h4, a one-move mate
    l0 = lines[off[R.I_MATE1] + 3][0]
    assert (text(l0), int(l0["kind"]), int(l0["pv_len"]), int(l0["reply_index"])) == (("d8h4", ""), F.BEST_MATE, 1, 0)
    # one move earlier g2g4 allows it: the last line, mated, with the reply d8h4
    ls = live(off[R.I_BLUNDER] + 2)
    assert len(ls) == 19 and text(ls[-1]) == ("g2g4", "d8h4") and int(ls[-1]["kind"]) == F.BEST_MATED
    assert (ls["kind"][:-1] == F.BEST_CP).all() and int(ls[-1]["pv_len"]) == 2
    assert (np.diff(ls["value"][:-1].astype(np.int64)) <= 0).all()  # values descending
    # every move allows a mate in one
    ls = live(off[R.I_MATED])
    assert len(ls) == 2 and (ls["kind"] == F.BEST_MATED).all() and ls["child"].tolist() == [1, 2]
    # the mating moves first in index order (the host finds one in this position, f7g7: after f7f8 the king
    # has h7; two mates in one group are in the hand-made arrays), the stalemating move worth 0
    ls = live(off[R.I_MOS])
    mates = ls[ls["kind"] == F.BEST_MATE]
    _, texts, ends = R.expand(GAMES[R.I_MOS][0], [], False)
    host_mates = [c + 1 for c, f in enumerate(ends[1:]) if f == F.END_NO_MOVES | F.END_CHECK]
    assert mates["child"].tolist() == host_mates and len(host_mates) >= 1 and "f7g7" in [text(l)[0] for l in mates]
    assert (ls["kind"][:len(mates)] == F.BEST_MATE).all() and (mates["pv_len"] == 1).all()
    stale = ls[(ls["kind"] == F.BEST_CP) & (ls["pv_len"] == 1)]
    assert len(stale) >= 1 and (stale["value"] == 0).all() and (stale["reply"] == 0).all()
    # 218 lines
    ls = live(off[R.I_MANY])
    assert len(ls) == 218 and sorted(ls["child"].tolist()) == list(range(1, 219))
    # the finished game's last ply: all-zero slots
    assert lines[-1].tobytes() == bytes(218 * N.LINE2_BYTES)
    assert int(out[-1]["kind"]) == F.BEST_NONE


# ---- 3. the variants ----

@pytest.fixture(scope="module")
def vsearched():
    from tests.test_gpu_vsearch2 import GAMES as VGAMES, net_of
    made = {v: F.Evaluator(F.Net.from_bytes_variant(net_of(v), v), 0) for v in (ZH, AT)}
    out = {}
    for v in (ZH, AT, KOTH):
        e = made[ZH] if v == ZH else made[AT]
        best2, off, kb, km = e.vsearch2(v, VGAMES[v], children=True)
        _, coff, moves, end = e.build_vchildren(v, VGAMES[v])
        out[v] = (e, VGAMES[v], best2, off, kb, coff, moves, end)
    yield out
    for e in made.values():
        e.close()


@pytest.mark.parametrize("v", [ZH, AT, KOTH], ids=["crazyhouse", "atomic", "kingOfTheHill"])
def test_vsearch2_lines_equals_the_order_over_the_children(vsearched, v):
    e, games, best2, off, kb, coff, moves, end = vsearched[v]
    k = 3
    got_out, got_off, lines = e.vsearch2_lines(v, games, k)
    assert got_out.tobytes() == best2.tobytes() and got_off.tobytes() == off.tobytes()
    want = M.lines_over_groups(end, moves, coff, as_tuples(kb), slot_offsets([k] * len(best2)), True)
    got = lines.reshape(-1)
    bad = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
    b2 = as_tuples(best2)
    for p in range(len(best2)):
        assert M.shared_of_line(as_tuples(lines[p][:1])[0]) == M.shared_of_best2(b2[p]), p
    nkid = np.diff(coff.astype(np.int64)) - 1
    if v == ZH:  # the full-pocket ply ranks beyond the fast path's 256 children
        assert nkid.max() == 306
        p = int(nkid.argmax())
        assert (lines[p]["kind"] != F.BEST_NONE).all() and len(set(lines[p]["child"].tolist())) == 3
        assert any("@" in F.vmove_uci(int(m)) for m in lines["move"].reshape(-1)) or \
            any("@" in F.vmove_uci(int(m)) for m in lines["reply"].reshape(-1) if m)
    assert {int(x) for x in lines["pv_len"].reshape(-1)} >= {1, 2}


# ---- 4. the scratch budget ----

BUDGET_CHILD = """
import sys
import numpy as np
import fishnet_amd as F
from tests.conftest import net_bytes
from tests.test_gpu_search2 import LONG_GAMES
ev = F.Evaluator(F.Net.from_bytes(net_bytes(1, 256, 0)), 0)
out, off, lines = ev.search2_lines(LONG_GAMES, 3)
np.save(sys.argv[1], out)
np.save(sys.argv[2], lines)
ev.close()
"""


def test_lines_do_not_depend_on_the_budget(ev, tmp_path):
    from tests.test_gpu_search2 import LONG_GAMES, MIN_RECORDS
    out, off, lines = ev.search2_lines(LONG_GAMES, 3)
    assert int(out["nodes"].astype(np.int64).sum()) > 4 * MIN_RECORDS  # several chunks at the smallest budget
    paths = [str(tmp_path / "out.npy"), str(tmp_path / "lines.npy")]
    env = dict(os.environ, FNNUE_SEARCH2_RECORDS="1")  # forced up to one ply's maximum
    subprocess.run([sys.executable, "-c", BUDGET_CHILD] + paths, cwd=ROOT, env=env, check=True, timeout=300)
    small_out, small_lines = np.load(paths[0]), np.load(paths[1])
    assert small_out.tobytes() == out.tobytes()
    assert small_lines.dtype == LINE2 and small_lines.tobytes() == lines.tobytes()


# ---- 5. the capacity protocol ----

def test_capacity_protocol_and_net_mismatch(ev, searched, vsearched):
    out = searched[0]
    text, fen_off, mv_off = F.pack_games(GAMES)
    plies, k = len(out), 3
    recs = np.full(plies * N.BEST2_BYTES, FILL, dtype=np.uint8)
    off = np.full(len(GAMES) + 1, 0xABABABAB, dtype=np.uint32)
    lines = np.full(plies * k * N.LINE2_BYTES, FILL, dtype=np.uint8)
    n, g = C.c_size_t(), C.c_size_t()
    args = (ev._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(GAMES), k, N.ptr(recs), plies, N.ptr(off),
            len(off), N.ptr(lines))
    assert N.lib.fnnue_search2_lines(*args, plies * k - 1, C.byref(n), C.byref(g)) == -10
    assert (n.value, g.value) == (plies, len(GAMES))
    assert (recs == FILL).all() and (off == 0xABABABAB).all() and (lines == FILL).all()  # nothing written
    assert N.lib.fnnue_search2_lines(*args, plies * k, C.byref(n), C.byref(g)) == 0
    assert recs.view(F.BEST2_DTYPE).tobytes() == out.tobytes()
    # a variant net's context on the chess entry, and the reverse
    zh = vsearched[ZH][0]
    with pytest.raises(F.FnnueError) as err:
        zh.search2_lines([(START, "e2e4")], 3)
    assert err.value.code == -4
    with pytest.raises(F.FnnueError) as err:
        ev.vsearch2_lines(ZH, [(R2_ZH_START, "e2e4")], 3)
    assert err.value.code == -4
    for bad in (0, 219):
        with pytest.raises(F.FnnueError) as err:
            ev.search2_lines(GAMES[:1], bad)
        assert err.value.code == -1


R2_ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
ZH_MATE = ("7k/6pp/8/8/8/8/8/K7[R] w - - 0 1", "R@e8")


# ---- 6. the engine actor ----

def make_channel(data, **kw):
    zh = F.synthesize_variant_net(5, 256, ZH)
    return B.channel(F.Net.from_bytes(data), 0, crazyhouse=F.Net.from_bytes_variant(zh, ZH), **kw)


@pytest.fixture(scope="module")
def chans(data):
    """Channels at (2 chess plies, 1 ply, never set, 2 plies for both settings), each with a crazyhouse net."""
    made = [make_channel(data, **kw) for kw in ({"analysis_plies": 2}, {"analysis_depth": 1}, {},
                                                {"analysis_plies": 2, "variant_analysis_plies": 2})]
    yield tuple(stub for stub, _ in made)
    for _, actor in made:
        actor.close()


def bodies_of(games, **kw):
    return [B.AcquireResponseBody(f"g{i}", fen, mv, variant="chess960" if fen == CHESS960 else "fromPosition", **kw)
            for i, (fen, mv) in enumerate(games)]


def strip(res, reply=True):
    from tests.test_gpu_search2 import strip as base
    return base(res, reply)


def lines_of(res):
    return [None if isinstance(rows, B.PositionFailed) else
            [r.lines and [(l.score.kind, l.score.value, tuple(l.pv), l.psqt, l.positional) for l in r.lines]
             for r in rows] for rows in res]


def trunc_div(a, b):
    return abs(a) // b * (1 if a >= 0 else -1)


def want_line(l, uci):
    kind = int(l["kind"])
    score = {F.BEST_MATE: ("mate", 1), F.BEST_MATED: ("mate", -1), F.BEST_LOST: ("mate", -1)}.get(
        kind, ("cp", trunc_div(int(l["value"]) * 100, NORM)))
    pv = (uci(int(l["move"])),) + ((uci(int(l["reply"])),) if int(l["pv_len"]) == 2 else ())
    return score + (pv, int(l["psqt"]), int(l["positional"]))


def test_actor_lines_against_search2_lines(chans, lines218):
    d2 = chans[0]
    out, off, lines = lines218
    for multipv in (3, 500):
        bodies = bodies_of(GAMES, multipv=multipv)
        res, pv = d2.go_lines_pv(bodies), d2.go_pv(bodies)
        assert strip(res) == strip(pv)  # the responses and the replies are go_pv()'s
        got = lines_of(res)
        for i, rows in enumerate(res):
            for q, r in enumerate(rows):
                ls = lines[off[i] + q]
                legal = int((ls["kind"] != F.BEST_NONE).sum())
                if legal == 0:
                    assert r.lines is None
                    continue
                assert got[i][q] == [want_line(l, F.move_uci) for l in ls[:min(multipv, 218, legal)]], (i, q)
                l0 = r.lines[0]  # line 0 is the response
                assert (l0.score, l0.pv, l0.psqt, l0.positional) == \
                    (r.score, [r.best_move] + ([r.reply] if r.reply else []), r.psqt, r.positional)
                assert r.depth == len(l0.pv) and r.matrix
        assert lines_of(d2.go_lines_pv(bodies)) == got  # the same call twice
    # the JSON parses, and its rows are the lines
    res = d2.go_lines_pv(bodies_of(GAMES, multipv=3))
    for rows in (res[R.I_BLUNDER], res[R.I_FINISHED], res[R.I_MOS]):
        parts = json.loads(B.into_analysis(rows))
        for r, part in zip(rows, parts):
            if not r.lines:
                assert part["depth"] == 0 and part["pv"] == [[[]]]
                continue
            assert part["depth"] == r.depth and len(part["pv"]) == len(r.lines) == len(part["score"])
            for l, pv_row, score_row in zip(r.lines, part["pv"], part["score"]):
                assert pv_row == [None] * r.depth + [l.pv] and score_row == [None] * r.depth + [{l.score.kind: l.score.value}]
    assert [len(r.lines) for r in res[R.I_MATED]] == [2] and len(res[R.I_MANY][0].lines) == 3


def test_actor_without_multipv_skipped_ids_and_other_work(chans):
    d2, d1, d0, _ = chans
    bodies = bodies_of(GAMES)  # multipv absent: no lines, go_pv()'s rows
    res = d2.go_lines_pv(bodies)
    assert all(r.lines is None for rows in res for r in rows) and strip(res) == strip(d2.go_pv(bodies))
    fen, mv = GAMES[R.I_MATE1]
    rows = d2.go_lines_pv([B.AcquireResponseBody("s", fen, mv, skip_positions=[1, 3], multipv=2)])[0]
    assert [r.skipped for r in rows] == [False, True, False, True]
    assert [r.lines and len(r.lines) for r in rows] == [2, None, 2, None] and rows[2].lines[0].pv[0] == rows[2].best_move
    # move work, and a crazyhouse batch while the variant setting is at 0 plies: unchanged, no lines
    move = [B.AcquireResponseBody("mv", START, "e2e4 e7e5", work="move")]
    zh = [B.AcquireResponseBody("zh", R2_ZH_START, F.random_vgame(1000, ZH, R2_ZH_START, 12), variant="crazyhouse",
                                multipv=3)]
    for body in (move, zh):
        got = d2.go_lines_pv(body)
        assert strip(got) == strip(d0.go(body)) and all(r.lines is None for r in got[0])


def test_actor_one_ply_and_zero_plies(chans):
    d2, d1, d0, _ = chans
    bodies = bodies_of(GAMES[4:], multipv=3)
    one, old = d1.go_lines_pv(bodies), d1.go_lines(bodies)
    assert strip(one) == strip(old) == strip(d1.go_pv(bodies))
    for rows, orows in zip(one, old):
        for r, o in zip(rows, orows):
            assert (r.lines is None) == (o.lines is None)
            if r.lines:
                assert [(l.score, l.pv, l.psqt, l.positional) for l in r.lines] == \
                    [(l.score, [l.move], l.psqt, l.positional) for l in o.lines]
    assert any(r.lines and len(r.lines) == 3 for rows in one for r in rows)
    zero = d0.go_lines_pv(bodies)
    assert all(r.lines is None for rows in zero for r in rows) and strip(zero) == strip(d0.go(bodies))
    # go_lines on the 2-plies channel is still a one-ply search with one-move lines
    again = d2.go_lines(bodies)
    assert strip(again) == strip(old) and lines_of_old(again) == lines_of_old(old)
    assert again[1][0].depth == 1 and isinstance(again[1][0].lines[0], B.PvLine)


def lines_of_old(res):
    return [[r.lines for r in rows] for rows in res]


def test_actor_crazyhouse_lines_hold_a_drop(chans, vsearched):
    d22 = chans[3]
    e = vsearched[ZH][0]
    games = [ZH_MATE, vsearched[ZH][1][3]]  # ... and the full-pocket game: a ply beyond the fast path
    bodies = [B.AcquireResponseBody(f"zh{i}", fen, mv, variant="crazyhouse", multipv=3)
              for i, (fen, mv) in enumerate(games)]
    res = d22.go_lines_pv(bodies)
    assert strip(res) == strip(d22.go_pv(bodies))
    out, off, lines = e.vsearch2_lines(ZH, games, 3)
    got = lines_of(res)
    for i, rows in enumerate(res):
        for q, r in enumerate(rows):
            ls = lines[off[i] + q]
            legal = int((ls["kind"] != F.BEST_NONE).sum())
            assert got[i][q] == ([want_line(l, F.vmove_uci) for l in ls[:legal]] if legal else None), (i, q)
    first = res[0][0]
    assert first.score == B.Score("mate", 1) and len(first.lines[0].pv) == 1 and "@" in first.lines[0].pv[0]
    assert any("@" in m for rows in res for r in rows for l in r.lines or () for m in l.pv)
    part = json.loads(B.into_analysis(res[0]))[0]
    assert part["pv"][0][-1] == first.lines[0].pv
    # a chess batch on this channel has its two-move lines too
    chess = d22.go_lines_pv(bodies_of(GAMES[6:7], multipv=2))
    assert len(chess[0][0].lines) == 2 and len(chess[0][0].lines[0].pv) == 2


def test_actor_capacity_and_failures(chans):
    d2 = chans[0]
    good = bodies_of(GAMES[5:7], multipv=3)
    bound = B.lines_bound(good)
    assert bound == 3 * (4 + 3)
    with pytest.raises(F.FnnueError) as err:
        d2.go_lines_pv(good, lines_cap=bound - 1)
    assert err.value.code == -10
    mixed = [good[0], B.AcquireResponseBody("bad", START, "e2e4 e7e5 e1e3", multipv=3), good[1]]
    res, alone = d2.go_lines_pv(mixed), d2.go_lines_pv(good)
    assert isinstance(res[1], B.PositionFailed) and res[1].code == -8
    assert strip([res[0], res[2]]) == strip(alone) and lines_of([res[0], res[2]]) == lines_of(alone)
    assert len(alone[0][0].lines) == 3 and len(alone[0][0].lines[0].pv) == 2


PIECES_CHILD = """
import json
import fishnet_amd as F
from fishnet_amd import backend as B
from tests.conftest import net_bytes
from tests.test_gpu_search2 import LONG_GAMES
from tests.test_gpu_multipv2 import bodies_of, lines_of, strip
stub, actor = B.channel(F.Net.from_bytes(net_bytes(1, 256, 0)), 0, analysis_plies=2)
res = stub.go_lines_pv(bodies_of(LONG_GAMES, multipv=3))
print("RESULT " + json.dumps({"rows": strip(res), "lines": lines_of(res), "stats": B.last_stats(actor)}))
actor.close()
"""


def test_piece_cuts_do_not_change_the_lines(chans):
    from tests.test_gpu_search2 import LONG_GAMES
    d2 = chans[0]
    res = d2.go_lines_pv(bodies_of(LONG_GAMES, multipv=3))
    assert B.last_stats(d2._actor)["pieces"] == 1
    env = dict(os.environ, FNNUE_BACKEND_PIECE_PLIES="1")  # forced up to its minimum: pieces of 16 plies
    out = subprocess.run([sys.executable, "-c", PIECES_CHILD], cwd=ROOT, env=env, check=True, capture_output=True,
                         text=True, timeout=300).stdout
    small = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert small["stats"]["pieces"] > 1
    assert small["rows"] == json.loads(json.dumps(strip(res)))
    assert small["lines"] == json.loads(json.dumps(lines_of(res)))

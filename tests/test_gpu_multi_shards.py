"""The one-process multi-GPU path (fishnet_amd/csrc/multi.cpp, MultiEvaluator)
at two and three shards, on one GPU: MultiEvaluator(net, [0] * nd,
replicas=True) makes nd contexts on device 0, and everything after creation
is the code `bench.py --gpus N` runs: the shard arithmetic, one host thread
per shard, the partition cuts on real shards, the per-context streams and the
error aggregation.  Everything is compared with the CPU oracle, bit-exact, and
never with a single-context Evaluator.  Not covered here (they need distinct
devices): ncclCommInitAll / ncclBroadcast, hipSetDevice between ordinals, and
the scaling curve."""
import re

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet, VariantOracleNet
from tests.conftest import net_bytes
from tests.test_multi import built_offset_tables

pytestmark = pytest.mark.gpu

ZH, AT = N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC
CHESS = {"hd128": (7, 128, 0), "hd1024": (1, 1024, 0)}
VARIANTS = {"zh256": ZH, "atomic256": AT}  # the smallest variant nets of the suite: seed 3, hd 256
SENT = -0x5A5A5A5B  # pre-fill of every output: a result never written stays this
GUARD = 64          # sentinel words kept before and after a host output


def _net_data(name):
    if name in CHESS:
        return net_bytes(*CHESS[name])
    return F.synthesize_variant_net(3, 256, VARIANTS[name])


@pytest.fixture(scope="module")
def multis(request):
    """multis(net name, nd): one replicated MultiEvaluator per (net, nd), all on device 0."""
    cache = {}

    def close_all():
        for m in cache.values():
            m.close()
        cache.clear()

    request.addfinalizer(close_all)

    def get(name, nd):
        if (name, nd) not in cache:
            data = _net_data(name)
            net = F.Net.from_bytes(data) if name in CHESS else F.Net.from_bytes_variant(data, VARIANTS[name])
            m = F.MultiEvaluator(net, [0] * nd, replicas=True)
            assert len(m) == nd and [m.ctx(i).device for i in range(nd)] == [0] * nd
            cache[(name, nd)] = m
        return cache[(name, nd)]

    return get


class Batch:
    """Inputs and their oracle results, computed once and never written to."""

    def __init__(self, oracle, pos, off=None):
        self.pos, self.off = pos, off
        self.ps, self.po, rc = oracle.eval_packed(pos, threads=8)
        assert rc == 0
        assert SENT not in self.ps and SENT not in self.po
        for a in (self.pos, self.ps, self.po) + (() if off is None else (off,)):
            a.setflags(write=False)

    def head(self, n):
        return self.pos[:n], self.ps[:n], self.po[:n]


@pytest.fixture(scope="module")
def data():
    """data(net name): positions / CHAIN / STAR batches (variant nets: positions / CHAIN) with oracle results."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        if name in CHESS:
            on = OracleNet(_net_data(name))
            # STAR: 12 roots with their children, spread over the plies of 12 playouts
            spos, soff = F.random_playouts(33, 12, mode=F.PLAYOUT_CHILDREN, threads=8)
            roots = np.linspace(0, len(soff) - 2, 12).astype(np.int64)
            parts = [spos[soff[g]:soff[g + 1]] for g in roots]
            soff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint32)
            d = {"pos": Batch(on, F.random_playouts(31, 3001, threads=8)),
                 "chain": Batch(on, *F.random_playouts(32, 60, mode=F.PLAYOUT_PLIES, threads=8)),
                 "star": Batch(on, np.concatenate(parts), soff)}
            assert len(d["pos"].pos) == 3001 and len(d["chain"].off) == 61 and len(d["star"].off) == 13
        else:
            v = VARIANTS[name]
            on = VariantOracleNet(_net_data(name), v)
            pos = F.random_vpositions(34, v, 1501, 160)
            if v == AT:  # the game ends with Nxf7 exploding the black king: its last record is a game-over record
                start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
                pos = np.concatenate([pos, F.game_vpositions(AT, start, "g1f3 e7e6 f3g5 f8e7 g5f7")])
            d = {"pos": Batch(on, pos), "chain": Batch(on, *F.random_vgames(35, v, 30, 60, threads=8))}
            assert len(d["chain"].off) == 31
        cache[name] = d
        return d

    return get


def guarded(n):
    buf = np.full(n + 2 * GUARD, SENT, np.int32)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool(np.all(buf[:GUARD] == SENT) and np.all(buf[len(buf) - GUARD:] == SENT))


def host_positions(m, pos, variant=False):
    """fnnue_multi_eval_[v]positions into sentinel-filled outputs with guard words around them."""
    pos = np.ascontiguousarray(pos)
    (bs, ps), (bo, po) = guarded(len(pos)), guarded(len(pos))
    call = N.lib.fnnue_multi_eval_vpositions if variant else N.lib.fnnue_multi_eval_positions
    N.check(call(m._h, N.ptr(pos), len(pos), N.ptr(ps), N.ptr(po)))
    assert guards_intact(bs) and guards_intact(bo)
    return ps, po


def host_groups(m, pos, off, mode):
    pos, off = np.ascontiguousarray(pos), np.ascontiguousarray(off, dtype=np.uint32)
    (bs, ps), (bo, po) = guarded(len(pos)), guarded(len(pos))
    N.check(N.lib.fnnue_multi_eval_groups(m._h, N.ptr(pos), len(pos), N.ptr(off), len(off) - 1, mode, N.ptr(ps),
                                          N.ptr(po)))
    assert guards_intact(bs) and guards_intact(bo)
    return ps, po


def same(got, ps, po, what=""):
    bad = np.nonzero((got[0] != ps) | (got[1] != po))[0]
    holes = np.nonzero((got[0] == SENT) | (got[1] == SENT))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first {bad[:5]}; never written: {holes[:5]}"


def spoil(pos, i):
    pos[i, 0] = (pos[i, 0] & 0xF0) | 7  # invalid piece code 7 on a1


def position_error(e, variant=False):
    """(shard, index) out of 'shard 2 (device 0): invalid position at index 2041'."""
    assert e.value.name == "FNNUE_E_POSITION"
    word = "invalid variant position" if variant else "invalid position"
    hit = re.search(r"shard (\d+) \(device 0\): " + word + r" at index (\d+)", str(e.value))
    assert hit, str(e.value)
    return int(hit.group(1)), int(hit.group(2))


# ---- positions, host entry ----

@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("net", list(CHESS))
def test_positions_host_every_count(multis, data, net, nd):
    """n around the shard count (empty shards) and 3001 (unequal shards): every
    index written where the oracle puts it, no hole at a seam, nothing outside,
    and the same bytes as the nd = 1 multi."""
    m, one, d = multis(net, nd), multis(net, 1), data(net)["pos"]
    for n in sorted({0, 1, 2, nd - 1, nd, nd + 1, 3001}):
        pos, ps, po = d.head(n)
        got = host_positions(m, pos)
        same(got, ps, po, f"n {n}")
        ref = host_positions(one, pos)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), n


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("net", list(VARIANTS))
def test_vpositions_host(multis, data, net, nd):
    """fnnue_multi_eval_vpositions; the atomic batch ends with an exploded-king
    record, in the last shard: (0, 0), not an error."""
    m, d = multis(net, nd), data(net)["pos"]
    total = len(d.pos)
    for n in sorted({1, nd - 1, nd, nd + 1, total}):
        pos, ps, po = d.head(n)
        same(host_positions(m, pos, variant=True), ps, po, f"n {n}")
    if VARIANTS[net] == AT:
        got = host_positions(m, d.pos, variant=True)
        assert total - 1 >= total * (nd - 1) // nd  # the record is in the last shard
        assert got[0][-1] == 0 and got[1][-1] == 0 and d.ps[-1] == 0 and d.po[-1] == 0
        assert np.any(got[1][total * (nd - 1) // nd:-1])


# ---- groups, host entry ----

def check_groups(m, nd, pos, off, ps, po, mode, what):
    got = host_groups(m, pos, off, mode)
    same(got, ps, po, what)
    cut = F.partition_groups(off, nd)
    assert cut[0] == 0 and cut[-1] == len(off) - 1
    for k in range(nd):
        # shard k is groups [cut[k], cut[k + 1]): whole groups, so no group straddles a cut
        lo, hi = int(off[cut[k]]), int(off[cut[k + 1]])
        assert lo <= hi
        assert np.array_equal(got[0][lo:hi], ps[lo:hi]) and np.array_equal(got[1][lo:hi], po[lo:hi]), (what, k)
        if k and cut[k] < len(off) - 1:
            # the first group after a cut: its first record is evaluated from scratch on the new
            # shard and the rest (a STAR parent's children, a CHAIN's next plies) relative to it
            g = int(cut[k])
            while g < len(off) - 1 and off[g + 1] == off[g]:
                g += 1
            if g < len(off) - 1:
                a, b = int(off[g]), int(off[g + 1])
                assert np.array_equal(got[0][a:b], ps[a:b]) and np.array_equal(got[1][a:b], po[a:b]), (what, k, g)
    return got


@pytest.mark.parametrize("mode", [F.GROUP_CHAIN, F.GROUP_STAR], ids=["chain", "star"])
@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("net", list(CHESS))
def test_groups_host_playouts_and_built_tables(multis, data, net, nd, mode):
    """Random-playout groups and the built offset tables (fewer groups than
    shards; empty groups at the start, the end and at each cut; one group
    with more than half of the positions; groups of one position), each shard's
    slice exact against the oracle."""
    m, d = multis(net, nd), data(net)
    b = d["chain" if mode == F.GROUP_CHAIN else "star"]
    check_groups(m, nd, b.pos, b.off, b.ps, b.po, mode, "playouts")
    for shards in (2, 3):  # the tables built for 2 and for 3 shards, on every nd
        for name, off in built_offset_tables(shards).items():
            # any grouping of any positions is valid input: CHAIN / STAR fall back to a refresh
            pos, ps, po = b.head(int(off[-1]))
            assert len(pos) == int(off[-1])
            check_groups(m, nd, pos, off, ps, po, mode, f"{name}/{shards}")
    if nd > 1:
        big = built_offset_tables(nd)["one_big_middle"]
        sizes = np.diff(big.astype(np.int64))
        assert sizes.max() * 2 > sizes.sum()
        cut = F.partition_groups(built_offset_tables(nd)["fewer_groups"], nd)
        assert np.count_nonzero(np.diff(cut.astype(np.int64)) == 0) >= 1  # an empty shard really occurs


@pytest.mark.parametrize("net", ["hd128", "zh256"])
def test_shard_of_only_empty_groups(multis, data, net):
    """Empty groups on a cut can leave a shard with groups and no position
    (off = 0 6 6 6 12 over three shards: the middle one is groups 1 and 2).
    That is an empty result, not a launch error; on the device entry the
    offsets of such a call are still checked."""
    import torch
    variant = net in VARIANTS
    off = np.array([0, 6, 6, 6, 12], np.uint32)
    assert list(F.partition_groups(off, 3)) == [0, 1, 3, 4]
    if not variant:
        pos, ps, po = data(net)["chain"].head(12)
        for nd in (1, 2, 3):
            for mode in (F.GROUP_CHAIN, F.GROUP_STAR):
                same(host_groups(multis(net, nd), pos, off, mode), ps, po, f"nd {nd} mode {mode}")
                assert host_groups(multis(net, nd), pos[:0], np.zeros(4, np.uint32), mode)[0].shape == (0,)
    ev = multis(net, 2).ctx(1)  # the single-context entries
    d_pos = torch.zeros(N.VPOS_BYTES if variant else N.POS_BYTES, dtype=torch.uint8, device="cuda")
    out = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    call = ev.eval_vgroups_device if variant else ev.eval_groups_device
    for offsets, ok in (([0, 0, 0], True), ([0, 0, 1], False), ([0, 1, 0], False)):
        d_off = torch.tensor(offsets, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        call(d_pos.data_ptr(), d_off.data_ptr(), 2, 0, F.GROUP_CHAIN, out[0:].data_ptr(), out[1:].data_ptr(), None)
        if ok:
            ev.check()
        else:
            with pytest.raises(F.FnnueError) as e:
                ev.check()
            assert e.value.name == "FNNUE_E_ARG"
        assert out.cpu().tolist() == [SENT, SENT]  # nothing is written


# ---- independence of nd ----

@pytest.mark.parametrize("net", list(CHESS))
def test_outputs_do_not_depend_on_nd(multis, data, net):
    d = data(net)
    outs = [host_positions(multis(net, nd), d["pos"].pos) for nd in (1, 2, 3)]
    outs += [(d["pos"].ps, d["pos"].po)]
    assert len({o[0].tobytes() for o in outs}) == 1 and len({o[1].tobytes() for o in outs}) == 1
    for key, mode in (("chain", F.GROUP_CHAIN), ("star", F.GROUP_STAR)):
        b = d[key]
        outs = [host_groups(multis(net, nd), b.pos, b.off, mode) for nd in (1, 2, 3)] + [(b.ps, b.po)]
        assert len({o[0].tobytes() for o in outs}) == 1 and len({o[1].tobytes() for o in outs}) == 1, key


# ---- device entries ----

class DeviceShards:
    """One shard per context, each in torch tensors of its own; outputs pre-filled with SENT."""

    def __init__(self, parts, offs=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.n = [len(p) for p in parts]
        self.pos = [torch.from_numpy(np.array(p)).to(self.dev) for p in parts]
        self.ng = None if offs is None else [len(o) - 1 for o in offs]
        self.off = None if offs is None else [
            torch.from_numpy(np.array(o, dtype=np.uint32).view(np.int32)).to(self.dev) for o in offs]
        self.refill()

    def refill(self):
        t = self.torch
        self.ps = [t.full((max(n, 1),), SENT, dtype=t.int32, device=self.dev) for n in self.n]
        self.po = [t.full((max(n, 1),), SENT, dtype=t.int32, device=self.dev) for n in self.n]

    def streams(self, own):
        """None: the contexts' own streams (so everything above must be done:
        synchronise).  Else a distinct torch stream per shard, ordered after
        the copies and fills above on torch's current stream."""
        t = self.torch
        if not own:
            t.cuda.synchronize(self.dev)
            return None
        self.keep = [t.cuda.Stream(self.dev) for _ in self.n]
        for s in self.keep:
            s.wait_stream(t.cuda.current_stream(self.dev))
        assert len({s.cuda_stream for s in self.keep}) == len(self.keep)
        return [s.cuda_stream for s in self.keep]

    def ptrs(self, tensors):
        return [t.data_ptr() if n else 0 for t, n in zip(tensors, self.n)]

    def results(self, i):
        n = self.n[i]
        return self.ps[i].cpu().numpy()[:n], self.po[i].cpu().numpy()[:n]


def position_splits(nd, n):
    """Unequal shard sizes over n positions; the second split has an empty shard."""
    if nd == 1:
        return [[n]]
    if nd == 2:
        return [[n // 3, n - n // 3], [0, n]]
    return [[1, n // 3, n - 1 - n // 3], [n // 2, 0, n - n // 2]]


def group_splits(nd, ng):
    return position_splits(nd, ng)


def run_positions_device(m, b, nd, variant):
    n = len(b.pos)
    for sizes in position_splits(nd, n):
        edges = np.concatenate([[0], np.cumsum(sizes)])
        sh = DeviceShards([b.pos[edges[i]:edges[i + 1]] for i in range(nd)])
        for own in (False, True):
            sh.refill()
            call = m.eval_vpositions_device if variant else m.eval_positions_device
            call(sh.ptrs(sh.pos), sh.n, sh.ptrs(sh.ps), sh.ptrs(sh.po), sh.streams(own))
            m.sync()
            for i in range(nd):
                lo, hi = edges[i], edges[i + 1]
                same(sh.results(i), b.ps[lo:hi], b.po[lo:hi], f"sizes {sizes} own streams {own} shard {i}")


def run_groups_device(m, b, nd, mode, variant):
    ng = len(b.off) - 1
    off = b.off.astype(np.int64)
    for counts in group_splits(nd, ng):
        gedges = np.concatenate([[0], np.cumsum(counts)])
        parts = [b.pos[off[gedges[i]]:off[gedges[i + 1]]] for i in range(nd)]
        offs = [(off[gedges[i]:gedges[i + 1] + 1] - off[gedges[i]]).astype(np.uint32) for i in range(nd)]
        sh = DeviceShards(parts, offs)
        assert sh.ng == list(counts)
        for own in (False, True):
            sh.refill()
            call = m.eval_vgroups_device if variant else m.eval_groups_device
            call(sh.ptrs(sh.pos), [t.data_ptr() if g else 0 for t, g in zip(sh.off, sh.ng)], sh.ng, sh.n, mode,
                 sh.ptrs(sh.ps), sh.ptrs(sh.po), sh.streams(own))
            m.sync()
            for i in range(nd):
                lo, hi = off[gedges[i]], off[gedges[i + 1]]
                same(sh.results(i), b.ps[lo:hi], b.po[lo:hi], f"groups {counts} own streams {own} shard {i}")


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("net", list(CHESS))
def test_device_entries_chess(multis, data, net, nd):
    """eval_positions_device and eval_groups_device (CHAIN, STAR): unequal
    shards, one of them empty, on the contexts' own streams and on one torch
    stream per shard; sync(), then every shard against the oracle."""
    m, d = multis(net, nd), data(net)
    run_positions_device(m, d["pos"], nd, variant=False)
    run_groups_device(m, d["chain"], nd, F.GROUP_CHAIN, variant=False)
    run_groups_device(m, d["star"], nd, F.GROUP_STAR, variant=False)


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("net", list(VARIANTS))
def test_device_entries_variant(multis, data, net, nd):
    """eval_vpositions_device and eval_vgroups_device, as above."""
    m, d = multis(net, nd), data(net)
    run_positions_device(m, d["pos"], nd, variant=True)
    run_groups_device(m, d["chain"], nd, F.GROUP_CHAIN, variant=True)


def test_dual_nets_per_shard(multis, data):
    """The benchmark's big + small pair: two multis of nd = 2 on device 0, and
    per shard one eval_groups_dual_device call of the big net's context i with
    the small net's context i; both nets' outputs equal their oracles."""
    import torch
    big, small = multis("hd1024", 2), multis("hd128", 2)
    b, bs = data("hd1024")["chain"], data("hd128")["chain"]
    assert np.array_equal(b.pos, bs.pos) and np.array_equal(b.off, bs.off)
    off = b.off.astype(np.int64)
    cut = F.partition_groups(b.off, 2).astype(np.int64)
    dev = torch.device("cuda", 0)
    outs = []
    for i in range(2):
        lo, hi = int(off[cut[i]]), int(off[cut[i + 1]])
        d_pos = torch.from_numpy(np.array(b.pos[lo:hi])).to(dev)
        d_off = torch.from_numpy((off[cut[i]:cut[i + 1] + 1] - lo).astype(np.int32)).to(dev)
        out = torch.full((4, hi - lo), SENT, dtype=torch.int32, device=dev)
        outs.append((d_pos, d_off, out))
    torch.cuda.synchronize(dev)
    for i, (d_pos, d_off, out) in enumerate(outs):
        big.ctx(i).eval_groups_dual_device(small.ctx(i), d_pos.data_ptr(), d_off.data_ptr(), len(d_off) - 1,
                                           len(d_pos), F.GROUP_CHAIN, out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr(), out[3].data_ptr(), None)
    big.sync()
    small.sync()
    for i, (_, _, out) in enumerate(outs):
        lo, hi = off[cut[i]], off[cut[i + 1]]
        o = out.cpu().numpy()
        same((o[0], o[1]), b.ps[lo:hi], b.po[lo:hi], f"big net, shard {i}")
        same((o[2], o[3]), bs.ps[lo:hi], bs.po[lo:hi], f"small net, shard {i}")


# ---- errors ----

@pytest.mark.parametrize("net", list(CHESS))
def test_host_errors_name_shard_and_whole_buffer_index(multis, data, net):
    """An invalid record in shard 2 of 3 (and in shards 1 and 2: the first
    failing shard is reported): FNNUE_E_POSITION, the message names the shard
    and the index in the caller's buffer; the next clean call is exact on
    every shard."""
    m, d = multis(net, 3), data(net)
    p = d["pos"]
    n = len(p.pos)
    for where, shard in (([2041], 2), ([2 * n // 3], 2), ([n - 1], 2), ([1777, 2041], 1), ([n // 3, n - 1], 1)):
        bad = p.pos.copy()
        for i in where:
            spoil(bad, i)
        assert shard == min(k for i in where for k in range(3) if n * k // 3 <= i < n * (k + 1) // 3)
        with pytest.raises(F.FnnueError) as e:
            host_positions(m, bad)
        assert position_error(e) == (shard, where[0])
        same(host_positions(m, p.pos), p.ps, p.po, "after the error")
    for key, mode in (("chain", F.GROUP_CHAIN), ("star", F.GROUP_STAR)):
        b = d[key]
        off = b.off.astype(np.int64)
        cut = F.partition_groups(b.off, 3).astype(np.int64)
        assert np.all(np.diff(off[cut]) > 3)
        in1, in2 = int(off[cut[1]]) + 2, int(off[cut[2]]) + 3  # whole-buffer indices inside shards 1 and 2
        for where, shard in (([in2], 2), ([int(off[cut[2]])], 2), ([in1, in2], 1)):
            bad = b.pos.copy()
            for i in where:
                spoil(bad, i)
            with pytest.raises(F.FnnueError) as e:
                host_groups(m, bad, b.off, mode)
            assert position_error(e) == (shard, where[0]), key
            same(host_groups(m, b.pos, b.off, mode), b.ps, b.po, f"{key} after the error")


@pytest.mark.parametrize("net", list(VARIANTS))
def test_host_errors_variant(multis, data, net):
    m, p = multis(net, 3), data(net)["pos"]
    n = len(p.pos)
    for where, shard in (([n - 9], 2), ([n // 3 + 5, n - 9], 1)):
        bad = p.pos.copy()
        for i in where:
            spoil(bad, i)
        with pytest.raises(F.FnnueError) as e:
            host_positions(m, bad, variant=True)
        assert position_error(e, variant=True) == (shard, where[0])
        same(host_positions(m, p.pos, variant=True), p.ps, p.po, "after the error")


@pytest.mark.parametrize("net", list(CHESS))
def test_device_errors_are_latched_per_shard_and_all_drained(multis, data, net):
    """An invalid record in shard 1 of 3 on the device entry: the enqueue is
    OK, sync() raises FNNUE_E_POSITION naming shard 1, shards 0 and 2 hold
    oracle-exact results (every context was drained), a second sync() is
    clean.  With invalid records in shards 1 and 2, shard 1 is reported and
    shard 2's error is cleared by the same sync()."""
    m, p = multis(net, 3), data(net)["pos"]
    edges = [0, 1000, 2000, 3001]
    for holes in ([1041], [1041, 2500]):
        bad = p.pos.copy()
        for i in holes:
            spoil(bad, i)
        sh = DeviceShards([bad[edges[i]:edges[i + 1]] for i in range(3)])
        for own in (False, True):
            sh.refill()
            m.eval_positions_device(sh.ptrs(sh.pos), sh.n, sh.ptrs(sh.ps), sh.ptrs(sh.po), sh.streams(own))  # OK
            with pytest.raises(F.FnnueError) as e:
                m.sync()
            assert e.value.name == "FNNUE_E_POSITION" and "shard 1 (device 0): " in str(e.value), str(e.value)
            m.sync()  # nothing stays latched on any shard
            for i in range(3):
                ok = np.ones(sh.n[i], dtype=bool)
                for h in holes:
                    if edges[i] <= h < edges[i + 1]:
                        ok[h - edges[i]] = False
                assert ok.all() == (i == 0 or (i == 2 and len(holes) == 1))
                ps, po = sh.results(i)
                lo, hi = edges[i], edges[i + 1]
                assert np.array_equal(ps[ok], p.ps[lo:hi][ok]) and np.array_equal(po[ok], p.po[lo:hi][ok]), (i, own)
                assert not np.any(ps[~ok]) and not np.any(po[~ok])  # an invalid record answers (0, 0)
    same(host_positions(m, p.pos), p.ps, p.po, "host entry after the device errors")

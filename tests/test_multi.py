"""Multi-GPU sharding: the partitioner (host), the fnnue_multi ABI's argument
checks (no GPU needed), a world_size-2 gloo run of the per-rank sharding of
grouped batches, and (-m gpu) the one-process multi-device path at ndev = 1
against the oracle (one MI355X per box; two and three shards on one GPU run
in tests/test_gpu_multi_shards.py, distinct devices in the driver's 8-GPU
bench)."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import fishnet_amd as F
from fishnet_amd import _native as N
from tests.conftest import ROOT, net_bytes


def test_partition_groups_balanced():
    rng = np.random.default_rng(5)
    for trial in range(20):
        sizes = rng.integers(0, 300, size=int(rng.integers(1, 2000)))
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        total, big = int(off[-1]), int(sizes.max())
        for parts in (1, 2, 3, 4, 7, 8, 64):
            cut = F.partition_groups(off, parts)
            assert cut[0] == 0 and cut[-1] == len(sizes)
            assert np.all(np.diff(cut.astype(np.int64)) >= 0)
            for k in range(1, parts):  # each boundary within half a group of the ideal split
                assert abs(int(off[cut[k]]) - total * k // parts) <= big
            shares = np.diff(off[cut].astype(np.int64))
            assert shares.sum() == total


def test_partition_groups_edge_cases():
    off = np.array([0, 5, 5, 5, 12], dtype=np.uint32)  # empty groups
    assert list(F.partition_groups(off, 1)) == [0, 4]
    cut = F.partition_groups(off, 8)  # more parts than groups: empty parts
    assert cut[0] == 0 and cut[-1] == 4 and np.all(np.diff(cut.astype(int)) >= 0)
    assert list(F.partition_groups(np.zeros(1, np.uint32), 3)) == [0, 0, 0, 0]
    for bad in (np.array([1, 5], np.uint32), np.array([0, 5, 3], np.uint32)):
        with pytest.raises(F.FnnueError) as e:
            F.partition_groups(bad, 2)
        assert e.value.name == "FNNUE_E_ARG"
    cut = np.zeros(2, np.uint32)
    assert N.lib.fnnue_partition_groups(N.ptr(off), 4, 0, N.ptr(cut)) == -1


def test_multi_create_argument_checks():
    import ctypes as C
    net = F.Net.from_bytes(net_bytes(7, 128, 0))
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert N.lib.fnnue_multi_create(net.handle, devs, 0, C.byref(h)) == -1  # ndev < 1
    rc = N.lib.fnnue_multi_create(net.handle, devs, 2, C.byref(h))
    # no GPU here -> FNNUE_E_DEVICE; with one, the duplicate device -> FNNUE_E_ARG
    assert rc in (-1, -5) and not h.value
    assert N.lib.fnnue_multi_sync(None) == -1


def test_multi_create_replicas_argument_checks():
    """fnnue_multi_create_replicas: the argument checks of fnnue_multi_create,
    except that an ordinal may repeat; without a GPU FNNUE_E_DEVICE, *out null."""
    import ctypes as C
    net = F.Net.from_bytes(net_bytes(7, 128, 0))
    create = N.lib.fnnue_multi_create_replicas
    devs = (C.c_int * 3)(0, 0, 0)
    for ndev in (0, -1):
        h = C.c_void_p(1)
        assert create(net.handle, devs, ndev, C.byref(h)) == -1 and not h.value
    h = C.c_void_p(1)
    assert create(None, devs, 3, C.byref(h)) == -1 and not h.value  # null net
    h = C.c_void_p(1)
    assert create(net.handle, None, 3, C.byref(h)) == -1 and not h.value  # null devices
    assert create(net.handle, devs, 3, None) == -1  # null out
    if F.device_count() == 0:
        h = C.c_void_p(1)
        assert create(net.handle, devs, 3, C.byref(h)) == -5 and not h.value
        assert "no HIP device" in N.lib.fnnue_last_error().decode()
        with pytest.raises(F.FnnueError) as e:
            F.MultiEvaluator(net, [0, 0], replicas=True)
        assert e.value.name == "FNNUE_E_DEVICE"
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 9
    assert N.lib.fnnue_abi_version() >> 16 == 3


def built_offset_tables(nd: int, unit: int = 6) -> dict:
    """Group-offset tables whose cuts over nd parts are awkward (also used on
    real shards by tests/test_gpu_multi_shards.py).  `unit` scales the sizes;
    the totals are multiples of nd * 2, so the ideal split points k / nd of the
    positions are whole numbers and can be hit exactly."""
    u = unit
    tables = {
        # fewer groups than parts: some parts must stay empty
        "one_group": [5 * u],
        "fewer_groups": [3 * u + 1] * (nd - 1),
        # empty groups at the start, at the end and exactly at every ideal split
        "empty_at_cuts": [0, 0] + sum(([u, u - 1, 1, 0, 0] for _ in range(nd)), []) + [0],
        # one group with more than half of all positions (no even split exists)
        "one_big_first": [9 * u, u, 1, u - 1, 2],
        "one_big_middle": [2, u, 1, 9 * u, u - 1, 3],
        "one_big_last": [u, 2, 1, u, 9 * u],
        # every group one position: every index is a boundary
        "singles": [1] * (4 * u * nd + 1),
        "only_empty": [0, 0, 0],
    }
    return {k: np.concatenate([[0], np.cumsum(v)]).astype(np.uint32) for k, v in tables.items()}


@pytest.mark.parametrize("parts", [1, 2, 3, 4, 8])
def test_partition_groups_built_tables(parts):
    """On the built tables: cuts are monotone, sit on group boundaries (by
    construction: they index off), each is the boundary nearest to its share
    of the positions among those not before the previous cut (so a cut that
    is one group off fails), and parts > ngroups leaves only empty extras."""
    for nd in (2, 3):
        for name, off in built_offset_tables(nd).items():
            ngroups, total = len(off) - 1, int(off[-1])
            cut = F.partition_groups(off, parts).astype(np.int64)
            assert len(cut) == parts + 1 and cut[0] == 0 and cut[-1] == ngroups, name
            assert np.all(np.diff(cut) >= 0), name
            o = off.astype(np.int64)
            for k in range(1, parts):
                target = total * k // parts
                best = np.abs(o[cut[k - 1]:] - target).min()
                assert abs(o[cut[k]] - target) == best, (name, k, cut.tolist())
            sizes = np.diff(o[cut])
            assert sizes.sum() == total and np.all(sizes >= 0), name
            nonempty_groups = int(np.count_nonzero(np.diff(o)))
            assert np.count_nonzero(sizes) <= nonempty_groups, name
            if parts > ngroups:  # the extra parts hold no group at all
                assert np.count_nonzero(np.diff(cut)) <= ngroups, name
                assert np.count_nonzero(np.diff(cut) == 0) >= parts - ngroups, name
    # the ideal split is hit exactly where a boundary sits on it, empty groups or not
    off = built_offset_tables(3)["empty_at_cuts"]
    cut = F.partition_groups(off, 3)
    assert [int(off[c]) for c in cut] == [0, 12, 24, 36]
    off = built_offset_tables(2)["singles"]
    assert list(F.partition_groups(off, 2)) == [0, 24, 49]
    # one group larger than an even share: it lands whole in one part
    off = built_offset_tables(2)["one_big_middle"]
    assert list(F.partition_groups(off, 2)) == [0, 3, 6]  # 9 | 54 + 5 + 3: boundary 9 is nearer to 35 than 63


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    import fishnet_amd as F
    from fishnet_amd import dist as D
    from oracle.oracle import OracleNet

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cpu = torch.device("cpu")
        pos, off = F.random_playouts(11, 40, mode=F.PLAYOUT_CHILDREN, threads=2)  # same batch on every rank
        g0, g1 = D.shard_groups(off, rank, world)
        lo, hi = int(off[g0]), int(off[g1])
        on = OracleNet(F.synthesize_net(7, 128, 0))  # each rank "evaluates" its shard (CPU stand-in)
        ps, po, rc = on.simd_eval_groups(pos[lo:hi], (off[g0:g1 + 1] - off[g0]).astype(np.uint32), F.GROUP_STAR,
                                         threads=1)
        assert rc == 0
        gps = D.gather_to_rank0(ps, cpu)
        gpo = D.gather_to_rank0(torch.from_numpy(po), cpu)
        q.put((rank, hi - lo, None if gps is None else (gps.tobytes(), gpo.tobytes())))
    finally:
        dist.destroy_process_group()


def test_two_rank_group_sharding_gloo():
    """Whole STAR groups split over 2 ranks by position count; the gathered
    results equal the whole batch evaluated in one piece."""
    from oracle.oracle import OracleNet
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    pos, off = F.random_playouts(11, 40, mode=F.PLAYOUT_CHILDREN, threads=2)
    assert res[0][1] + res[1][1] == len(pos)
    assert abs(res[0][1] - res[1][1]) < 400  # balanced by positions (groups are <= ~60 positions)
    ps, po, rc = OracleNet(F.synthesize_net(7, 128, 0)).eval_packed(pos)
    gps, gpo = res[0][2]
    assert np.frombuffer(gps, np.int32).tolist() == ps.tolist()
    assert np.frombuffer(gpo, np.int32).tolist() == po.tolist()


@pytest.mark.gpu
def test_multi_single_device_matches_oracle():
    """fnnue_multi at ndev = 1 (RCCL communicator + broadcast of the image to
    itself): host and device entry points bit-exact against the oracle."""
    import torch
    from oracle.oracle import OracleNet
    data = net_bytes(1, 1024, 0)
    m = F.MultiEvaluator(F.Net.from_bytes(data), [0])
    on = OracleNet(data)
    try:
        pos = F.random_playouts(21, 30000, threads=8)
        ps, po = m.eval_positions(pos)
        ops, opo, rc = on.eval_packed(pos, threads=8)
        assert rc == 0 and np.array_equal(ps, ops) and np.array_equal(po, opo)
        for mode, pm, count in ((F.GROUP_CHAIN, F.PLAYOUT_PLIES, 300), (F.GROUP_STAR, F.PLAYOUT_CHILDREN, 30)):
            gpos, off = F.random_playouts(22, count, mode=pm, threads=8)
            gs, go = m.eval_groups(gpos, off, mode)
            ops, opo, rc = on.eval_packed(gpos, threads=8)
            assert np.array_equal(gs, ops) and np.array_equal(go, opo)
        dev = torch.device("cuda", 0)
        d_pos = torch.from_numpy(pos).to(dev)
        d_ps = torch.zeros(len(pos), dtype=torch.int32, device=dev)
        d_po = torch.zeros(len(pos), dtype=torch.int32, device=dev)
        cur = [torch.cuda.current_stream(dev).cuda_stream]  # ordered after the zero fills above
        m.eval_positions_device([d_pos.data_ptr()], [len(pos)], [d_ps.data_ptr()], [d_po.data_ptr()], cur)
        m.sync()
        assert np.array_equal(d_ps.cpu().numpy(), ps) and np.array_equal(d_po.cpu().numpy(), po)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        d_g = torch.from_numpy(gpos).to(dev)
        d_gs = torch.zeros(len(gpos), dtype=torch.int32, device=dev)
        d_go = torch.zeros(len(gpos), dtype=torch.int32, device=dev)
        m.eval_groups_device([d_g.data_ptr()], [d_off.data_ptr()], [len(off) - 1], [len(gpos)], F.GROUP_STAR,
                             [d_gs.data_ptr()], [d_go.data_ptr()], cur)
        m.sync()
        assert np.array_equal(d_gs.cpu().numpy(), gs) and np.array_equal(d_go.cpu().numpy(), go)
        assert m.ctx(0).device == 0
    finally:
        m.close()

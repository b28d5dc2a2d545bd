"""The value domain of the layer stacks on the CPU (tests/stack_nets.py): the
crafted nets reach what they are built to reach, asserted from the numpy
restatement alone (tests/refpy.py, traced), and the three references (scalar
oracle, SIMD baseline on both ISAs, refpy) agree on every record of every
crafted net, so that the oracle can be the yardstick for the GPU on this
domain (tests/test_gpu_stack_domain.py).  No GPU."""
import json

import numpy as np
import pytest

from fishnet_amd import _native as N
from oracle import oracle as O
from tests import corpus as Cp
from tests import refpy
from tests import stack_nets as S


@pytest.fixture(scope="module", params=S.FAMILY, ids=S.net_id)
def net(request):
    """One crafted net: its bytes, the oracle's net, and refpy's traced results on every record."""
    spec = request.param
    data = S.make(spec)
    ref = refpy.RefNet(data)
    rec = S.records()
    ps, po = np.zeros(len(rec), np.int64), np.zeros(len(rec), np.int64)
    y, z = np.zeros((len(rec), S.L2), np.int64), np.zeros((len(rec), S.L3), np.int64)
    for i, p in enumerate(rec):
        ps[i], po[i], y[i], z[i] = refpy.evaluate(ref, *O.unpack(p), trace=True)
    del ref
    for a in (ps, po, y, z):
        a.setflags(write=False)
    return {"spec": spec, "oracle": O.OracleNet(data), "ps": ps, "po": po, "y": y, "z": z,
            "bucket": Cp.buckets(rec)}


@pytest.fixture(params=["avx2", "avx512"])
def simd_isa(request):
    want = request.param == "avx512"
    got = O.lib.cpu_simd_set_isa(int(want))
    if want and not got:
        pytest.skip("host has no AVX-512 VNNI")
    yield request.param
    O.lib.cpu_simd_set_isa(1)


def _occurs_in(values, buckets, target) -> int:
    """The number of buckets in which `target` occurs among `values` (records x outputs)."""
    return len(set(buckets[np.nonzero((values == target).any(axis=1))[0]].tolist()))


def test_the_target_orders_hold_every_band():
    """Any 15 consecutive y targets hold every |y| band, so each bucket of a boundary net does."""
    n = len(S.Y_ORDER)
    assert sorted(S.Y_ORDER) == sorted(S.Y_TARGETS) and n == 49
    for i in range(n):
        assert set(S.band_of([S.Y_ORDER[(i + j) % n] for j in range(S.L2 - 1)]).tolist()) == set(range(5))
    # the bands' edges are where the arithmetic says: 8160^2 >> 19 is the first 127, 46341^2 is the
    # first square above int32, 65536^2 the first above uint32
    assert (8159 ** 2 >> 19, 8160 ** 2 >> 19) == (126, 127)
    assert 46340 ** 2 < 1 << 31 <= 46341 ** 2 and 65535 ** 2 < 1 << 32 == 65536 ** 2
    assert 223696 * 9600 < 1 << 31 <= 223697 * 9600


def test_value_domain_is_reached(net):
    """From refpy's trace alone.  Boundary nets: every bucket is evaluated, y is the target of its
    (bucket, output) slot on every record; each listed y target occurs in at least two buckets and
    every bucket holds every band; z likewise for the kinds that fix it; fc_1 and fc_2 see all
    inputs at 127 where the kind says so.  Extreme nets: every |y| band holds at least 2 % of the
    fc_0 activations, and negative y15 that are no multiple of 8128 occur in every bucket."""
    family, hd, kind, _ = net["spec"]
    y, z, bucket = net["y"], net["z"], net["bucket"]
    assert set(bucket.tolist()) == set(range(8))
    act = y[:, :15]
    if family == "extreme":
        frac = np.bincount(S.band_of(act).ravel(), minlength=5) / act.size
        print(f"hd {hd}: band fractions {frac.round(4).tolist()}")
        assert frac.min() >= 0.02
        for b in range(8):
            y15 = y[bucket == b, 15]
            assert ((y15 < 0) & (y15 % 8128 != 0)).any(), b
        return
    assert np.array_equal(y, S.y_targets(kind)[bucket])
    if kind != "fc1_sat":
        for b in range(8):
            assert set(S.band_of(act[bucket == b]).ravel().tolist()) == set(range(5)), b
    if kind == "fc1_sat":
        assert act.min() >= 8192  # SqrCReLU and CReLU both at 127 in all 30 fc_1 inputs
        for t in S.Y_SATURATED:
            assert _occurs_in(act, bucket, t) >= 2, t
    else:
        for t in S.Y_TARGETS:
            assert _occurs_in(act, bucket, t) >= 2, t
    want15 = {S.FWD_TARGETS[(S.KINDS[kind][2] + b) % len(S.FWD_TARGETS)] for b in range(8)}
    assert set(y[:, 15].tolist()) == want15 and len(want15) == 8
    zt = S.z_targets(kind)
    if zt is not None:
        assert np.array_equal(z, zt[bucket])
        for t in S.Z_SATURATED if kind == "fc2_sat" else S.Z_TARGETS:
            assert _occurs_in(z, bucket, t) >= 2, t
    if kind == "fc2_sat":
        assert z.min() >= 8128  # all 32 fc_2 inputs at 127


def test_fwd_targets_over_the_kinds():
    """Output 15 has 8 slots per net and 18 targets: the three w0 kinds together hold all but one,
    the first four kinds all of them, and over the six kinds every bucket meets a negative y15 that
    is no multiple of 8128.  From refpy, one record per bucket (y does not depend on HD)."""
    rec = S.records()
    bucket = Cp.buckets(rec)
    first = [int(np.argmax(bucket == b)) for b in range(8)]
    seen, neg = {}, np.zeros(8, dtype=bool)
    for kind in S.KINDS:
        ref = refpy.RefNet(S.boundary_net(128, kind))
        y15 = [int(refpy.evaluate(ref, *O.unpack(rec[i]), trace=True)[2][15]) for i in first]
        seen[kind] = set(y15)
        neg |= np.array([v < 0 and v % 8128 != 0 for v in y15])
    assert len(set().union(*(seen[k] for k in S.W0_KINDS))) == 17
    assert set().union(*(seen[k] for k in list(S.KINDS)[:4])) == set(S.FWD_TARGETS)
    assert neg.all()
    # the HD 3072 net (w0=-128) alone: both sides of the int32 edge of y * 9600, and the far end
    assert {223696, -223696, 223697, -223697, 40_000_000, -40_000_000} <= seen["w0=-128"]


def test_references_agree(net, simd_isa):
    """Oracle == SIMD baseline == refpy on every record; oracle == SIMD along CHAIN / STAR groups."""
    on = net["oracle"]
    rec = S.records()
    a, b = on.eval_packed(rec, threads=4), on.simd_eval_packed(rec, threads=4)
    assert a[2] == b[2] == 0
    assert np.array_equal(a[0], net["ps"]) and np.array_equal(a[1], net["po"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for pos, off in (S.chains(300), Cp.sweep_groups(rec)):
        want = on.eval_packed(pos, threads=4)
        for mode in (N.GROUP_CHAIN, N.GROUP_STAR):
            got = on.simd_eval_groups(pos, off, mode, threads=4)
            assert want[2] == got[2] == 0
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


def test_psqt_wraps_only_in_the_wrap_nets(net):
    """The +-2^24 nets keep every PSQT sum inside int32 (refpy's reduction mod 2^32 changes nothing
    there); the wrap nets do leave it, and the halved difference still covers the int32 range."""
    _, _, _, psqt = net["spec"]
    ps = net["ps"]
    if psqt == S.PSQT_WRAP:
        assert np.abs(ps).max() > 1 << 29 and ps.min() < 0 < ps.max()
    elif psqt == S.PSQT_24:
        assert 1 << 24 < np.abs(ps).max() < 1 << 29


def test_golden_digest(net):
    """The oracle's results on every crafted net are pinned: a change to the reference shows."""
    golden = json.load(open(S.GOLDEN))["sha256"]
    ps, po, rc = net["oracle"].eval_packed(S.records(), threads=4)
    assert rc == 0
    assert S.digest(ps, po) == golden[S.net_id(net["spec"])]
    assert set(golden) == {S.net_id(s) for s in S.FAMILY}

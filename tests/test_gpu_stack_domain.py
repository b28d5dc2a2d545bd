"""The value domain of the layer stacks on the GPU (tests/stack_nets.py): boundary
nets that put every fc_0 / fc_1 sum on a chosen edge (CReLU and SqrCReLU edges,
the square leaving int32 and uint32, y * 9600 leaving int32, negative fwd
quotients, all inputs at 127 against weights of 127 / -128, fc_1 padding
weights, |fc_0 sum| = 126 * 128 * HD), nets with uniform int8 stack weights over
a real FT, and PSQT weights of +-2^24 or over all of int32 (sums wrap mod 2^32),
bit-exact against the CPU oracle on every path that ends in stack_kernel or
produces psqt_part.  tests/test_stack_domain.py shows on the CPU that the nets
reach those values and that the references agree there.  Run on an MI355X with
-m gpu; nothing runs at workload size."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet, VariantOracleNet
from tests import corpus as Cp
from tests import stack_nets as S
from tests.test_gpu_corpus import assert_equal, groups_device

pytestmark = pytest.mark.gpu

MODES = (N.GROUP_CHAIN, N.GROUP_STAR)
IMPLS = (N.FT_SLICED, N.FT_GATHER)  # groups: ft_segments / ft_groups


@pytest.fixture(scope="module")
def inputs():
    """name -> (records, offsets or None), built once and never changed: the records of the CPU
    test, chains of lengths 3..10 below and above the small-plan size, unrelated groups."""
    rec = S.records()
    out = {"records": (rec, None), "chains<=2048": S.chains(600), "chains>2048": S.chains(2600, seed=32),
           "sweep": Cp.sweep_groups(rec)}
    assert len(out["chains<=2048"][0]) <= 2048 < len(out["chains>2048"][0])
    for pos, off in out.values():
        pos.setflags(write=False)
        if off is not None:
            off.setflags(write=False)
    return out


@pytest.fixture(scope="module", params=S.FAMILY, ids=S.net_id)
def net(request, inputs):
    """One crafted net: (evaluator, the oracle's results by input name)."""
    data = S.make(request.param)
    on = OracleNet(data)
    want = {}
    for name, (pos, _) in inputs.items():
        ps, po, rc = on.eval_packed(pos, threads=8)
        assert rc == 0
        want[name] = (ps, po)
    del on
    ev = F.Evaluator(F.Net.from_bytes(data), 0)
    yield ev, want
    ev.close()


def positions_device(ev, pos):
    import torch
    d = torch.from_numpy(np.array(pos)).cuda()
    out = torch.full((2, len(pos)), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev.eval_positions_device(d.data_ptr(), len(pos), out[0].data_ptr(), out[1].data_ptr(), None)
    ev.check()
    o = out.cpu().numpy()
    return o[0], o[1]


def test_positions(net, inputs):
    """FT_SLICED and FT_GATHER, host and device entry == the oracle on every record."""
    ev, want = net
    pos = inputs["records"][0]
    try:
        for impl in IMPLS:
            ev.set_ft_impl(impl)
            assert_equal(ev.eval_positions(pos), want["records"], f"impl {impl} host")
            assert_equal(positions_device(ev, pos), want["records"], f"impl {impl} device")
    finally:
        ev.set_ft_impl(N.FT_AUTO)


def test_groups(net, inputs):
    """CHAIN and STAR through ft_segments (both plan sizes) and ft_groups, host and device entry."""
    ev, want = net
    try:
        for impl in IMPLS:
            ev.set_ft_impl(impl)
            for name in ("chains<=2048", "chains>2048", "sweep"):
                pos, off = inputs[name]
                for mode in MODES:
                    assert_equal(ev.eval_groups(pos, off, mode), want[name], f"{name} impl {impl} mode {mode} host")
                    assert_equal(groups_device(ev, pos, off, mode), want[name], f"{name} impl {impl} mode {mode} device")
    finally:
        ev.set_ft_impl(N.FT_AUTO)


def test_extreme_dual_net(inputs):
    """fnnue_eval_groups_dual_device with the (1024, 128) extreme-weight pair on the chains."""
    made = []
    try:
        for hd in (1024, 128):
            data = S.extreme_net(hd)
            made.append((F.Evaluator(F.Net.from_bytes(data), 0), OracleNet(data)))
        (big, obig), (small, osmall) = made
        for name in ("chains<=2048", "chains>2048"):
            pos, off = inputs[name]
            wb, ws = obig.eval_packed(pos, threads=8), osmall.eval_packed(pos, threads=8)
            assert wb[2] == ws[2] == 0
            for mode in MODES:
                ps, po, ps2, po2 = big.eval_groups_dual(small, np.array(pos), np.array(off), mode)
                assert_equal((ps, po), wb[:2], f"{name} mode {mode} big")
                assert_equal((ps2, po2), ws[:2], f"{name} mode {mode} small")
    finally:
        for ev, _ in made:
            ev.close()


@pytest.mark.parametrize("psqt", [S.PSQT_24, S.PSQT_WRAP])
@pytest.mark.parametrize("variant", [N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC])
def test_variant_psqt(variant, psqt):
    """The variant tile's psqt_part: a boundary net over the variant's feature set (HD 256), PSQT
    weights of +-2^24 or over all of int32, against the variant oracle; from scratch and along
    chains and unrelated groups, host and device entry."""
    data = S.boundary_net(256, "w0=0", psqt, variant)
    ev, on = F.Evaluator(F.Net.from_bytes_variant(data, variant), 0), VariantOracleNet(data, variant)
    try:
        rec = Cp.variant_corpus(variant)[::13].copy()
        batches = [("corpus", rec, Cp.sweep_groups(rec)[1]), ("chains",) + S.vchains(variant, 600)]
        for name, pos, off in batches:
            ps, po, rc = on.eval_packed(pos, threads=8)
            assert rc == 0
            if psqt == S.PSQT_WRAP:
                assert np.abs(ps).max() > 1 << 29
            assert name != "corpus" or set(Cp.buckets(pos).tolist()) == set(range(8))
            assert_equal(ev.eval_vpositions(pos), (ps, po), f"{name} from scratch")
            for mode in MODES:
                assert_equal(ev.eval_vgroups(pos, off, mode), (ps, po), f"{name} mode {mode} host")
                assert_equal(groups_device(ev, pos, off, mode, variant=True), (ps, po), f"{name} mode {mode} device")
    finally:
        ev.close()


def _with_w1_column(data: bytes, o: int) -> bytes:
    """w1[:, o] = 64 in every bucket: one step of fc_1 input o moves every z by one CReLU step."""
    im = S.Image(data)
    for b in range(S.STACKS):
        im.w1[b][:, o] = 64
    return im.bytes()


@pytest.mark.parametrize("kind,edge", [("fc1_zero", 8159), ("w0=0", 223696)])
def test_a_wrong_activation_is_noticed(inputs, kind, edge):
    """What the boundary nets are for: one b0 of the evaluator's net moves by one across an edge
    (SqrCReLU 126 -> 127 at y = 8159 -> 8160; y15 = 223696 -> 223697, where y * 9600 leaves int32).
    The results of exactly the records of that bucket change, to the oracle's value for the new
    net.  For the activation, fc_1 column o is 64 in both nets, so that the step of one in its
    input reaches z >> 6."""
    hd = 128
    pos = inputs["records"][0]
    bucket = Cp.buckets(pos)
    data = S.boundary_net(hd, kind)
    b, o = (int(v) for v in np.argwhere(S.y_targets(kind) == edge)[0])
    assert (o == S.L2 - 1) == (edge == 223696)
    if o < S.L2 - 1:
        data = _with_w1_column(data, o)
    im = S.Image(data)
    assert int(im.b0[b][o]) == edge - S.KINDS[kind][0] * S.X * hd
    im.b0[b][o] += 1
    moved = im.bytes()
    before, after = OracleNet(data).eval_packed(pos, threads=8), OracleNet(moved).eval_packed(pos, threads=8)
    assert before[2] == after[2] == 0
    changed = (before[0] != after[0]) | (before[1] != after[1])
    assert np.array_equal(changed, bucket == b) and 39 <= changed.sum() < len(pos)
    for d, want in ((data, before), (moved, after)):
        ev = F.Evaluator(F.Net.from_bytes(d), 0)
        try:
            for impl in IMPLS:
                ev.set_ft_impl(impl)
                assert_equal(ev.eval_positions(pos), want[:2], f"impl {impl}")
        finally:
            ev.close()

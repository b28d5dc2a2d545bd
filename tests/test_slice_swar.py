"""SWAR eligibility per 64-column slice, host side: the slice
bounds against a numpy restatement over the raw file bytes, the heavy-tailed
synthetic net (FNNUE_SYNTH_HEAVY) and the argument checks of the new calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N

CZH, ATOMIC = F.VARIANT_CRAZYHOUSE, F.VARIANT_ATOMIC
ROWS = {0: 704, CZH: 864, ATOMIC: 704}  # feature rows per own-king block

CASES = [(0, hd, flags) for hd in (128, 512, 1024) for flags in (0, N.SYNTH_WRAP, N.SYNTH_HEAVY)] + \
        [(v, 256, flags) for v in (CZH, ATOMIC) for flags in (0, N.SYNTH_HEAVY)]


@functools.lru_cache(maxsize=None)
def synth(variant: int, hd: int, flags: int, seed: int = 5) -> bytes:
    return F.synthesize_net(seed, hd, flags) if variant == 0 else F.synthesize_variant_net(seed, hd, variant, flags)


def load(data: bytes, variant: int) -> F.Net:
    return F.Net.from_bytes(data) if variant == 0 else F.Net.from_bytes_variant(data, variant)


def ft_tables(data: bytes, variant: int, hd: int):
    """(bias [hd], weights [blocks][rows][hd]) of a plain-format file, as int64."""
    blocks = 32 if variant == 0 else 64
    o = 12 + int(np.frombuffer(data, "<u4", 1, 8)[0]) + 4
    bias = np.frombuffer(data, "<i2", hd, o).astype(np.int64)
    w = np.frombuffer(data, "<i2", blocks * ROWS[variant] * hd, o + 2 * hd)
    return bias, w.reshape(blocks, ROWS[variant], hd).astype(np.int64)


def numpy_slice_bounds(data: bytes, variant: int, hd: int) -> np.ndarray:
    """Per king block and column: |bias + own-king row| + the 31 largest |w| of
    the other rows; second-half columns doubled; the maximum over a slice's
    even first-half columns and all its second-half columns."""
    bias, w = ft_tables(data, variant, hd)
    col = np.zeros(hd, dtype=np.int64)
    for kb in range(w.shape[0]):
        krow = 640 + 8 * (7 - (kb >> 2)) + (7 - (kb & 3)) if variant == 0 else 640 + kb
        a = np.abs(w[kb])
        a[krow] = 0
        top = -np.partition(-a, 30, axis=0)[:31]
        col = np.maximum(col, np.abs(bias + w[kb, krow]) + top.sum(axis=0))
    half = hd // 2
    out = np.zeros(hd // 64, dtype=np.int64)
    for s in range(hd // 64):
        out[s] = max(col[32 * s:32 * s + 32:2].max(), 2 * col[half + 32 * s:half + 32 * s + 32].max())
    return out


@pytest.mark.parametrize("variant,hd,flags", CASES)
def test_slice_bounds_match_numpy(variant, hd, flags):
    data = synth(variant, hd, flags)
    net = load(data, variant)
    got = net.slice_bounds()
    assert got.dtype == np.int32 and got.shape == (hd // 64,)
    assert np.array_equal(got.astype(np.int64), numpy_slice_bounds(data, variant, hd))
    assert int(got.max()) == net.accumulator_bound()
    if flags == N.SYNTH_HEAVY:
        heavy = np.arange(hd // 64) % 3 == 1
        assert heavy.any() and (got[heavy] >= 32768).all() and (got[~heavy] < 32768).all()
    elif flags == 0:
        assert (got < 32768).all()


@pytest.mark.parametrize("variant,hd", [(0, 128), (0, 512), (0, 1024), (CZH, 256), (ATOMIC, 256)])
def test_heavy_net_overwrites_one_column_per_heavy_slice(variant, hd):
    """Every third slice gets one same-sign column with a zero bias, second-half
    (|w| 520..540) and even first-half (|w| 1100..1300) in turn; every other
    column is the ordinary net's; the overwrite is deterministic."""
    plain, heavy = synth(variant, hd, 0), synth(variant, hd, N.SYNTH_HEAVY)
    assert heavy == (F.synthesize_net(5, hd, N.SYNTH_HEAVY) if variant == 0
                     else F.synthesize_variant_net(5, hd, variant, N.SYNTH_HEAVY))
    o = 12 + int(np.frombuffer(plain, "<u4", 1, 8)[0]) + 4
    oh = 12 + int(np.frombuffer(heavy, "<u4", 1, 8)[0]) + 4
    assert len(plain) - o == len(heavy) - oh  # the descriptions name their flags
    (b0, w0), (b1, w1) = ft_tables(plain, variant, hd), ft_tables(heavy, variant, hd)
    w0, w1 = w0.reshape(-1, hd), w1.reshape(-1, hd)
    changed = np.nonzero((w0 != w1).any(axis=0))[0]
    half = hd // 2
    want = list(range(1, hd // 64, 3))
    assert len(changed) == len(want)
    kinds = {}
    for c in changed:
        s = (c if c < half else c - half) // 32
        kinds[s] = c >= half
        mag = np.abs(w1[:, c])
        assert b1[c] == 0 and (np.sign(w1[:, c]) == np.sign(w1[0, c])).all()
        if c >= half:
            assert 520 <= mag.min() and mag.max() <= 540
        else:
            assert c % 2 == 0 and 1100 <= mag.min() and mag.max() <= 1300
    assert sorted(kinds) == want
    assert [kinds[s] for s in want] == [k % 2 == 0 for k in range(len(want))]  # second-half first, then in turn
    keep = np.ones(hd, bool)
    keep[changed] = False
    assert np.array_equal(b0[keep], b1[keep])
    assert plain[o + 2 * hd + 2 * w0.size:] == heavy[oh + 2 * hd + 2 * w1.size:]  # PSQT and the layer stacks


def test_heavy_slices_above_bit_32():
    b = F.Net.from_bytes(synth(0, 3072, N.SYNTH_HEAVY)).slice_bounds()
    heavy = np.arange(48) % 3 == 1
    assert len(b) == 48 and (b[heavy] >= 32768).all() and (b[~heavy] < 32768).all() and heavy[34:].any()


@pytest.mark.parametrize("variant,hd", [(0, 512), (CZH, 256)])
def test_heavy_leb128_net_parses_to_the_same_weights(variant, hd):
    plain = synth(variant, hd, N.SYNTH_HEAVY)
    leb = synth(variant, hd, N.SYNTH_HEAVY | N.SYNTH_LEB128)
    assert len(leb) < len(plain)
    a, b = load(plain, variant), load(leb, variant)
    assert np.array_equal(a.image(), b.image())
    assert np.array_equal(a.slice_bounds(), b.slice_bounds())


def test_new_calls_check_their_arguments():
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 3
    net = F.Net.from_bytes(synth(0, 512, 0))
    out = (C.c_int32 * 8)()
    n = C.c_size_t()
    E_ARG = -1
    assert N.lib.fnnue_net_slice_bounds(None, out, 8, C.byref(n)) == E_ARG
    assert N.lib.fnnue_net_slice_bounds(net.handle, None, 8, C.byref(n)) == E_ARG
    assert N.lib.fnnue_net_slice_bounds(net.handle, out, 8, None) == E_ARG
    n.value = 0
    assert N.lib.fnnue_net_slice_bounds(net.handle, out, 7, C.byref(n)) == E_ARG
    assert n.value == 8  # the size needed is reported
    assert N.lib.fnnue_net_slice_bounds(net.handle, out, 8, C.byref(n)) == 0 and n.value == 8
    assert list(out) == list(net.slice_bounds())
    el, en, ns = C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert N.lib.fnnue_ctx_swar_slices(None, C.byref(el), C.byref(en), C.byref(ns)) == E_ARG
    assert N.lib.fnnue_ctx_set_swar_slices(None, 1) == E_ARG

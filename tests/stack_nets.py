"""Crafted nets over the value domain of the layer stacks (test-only, numpy).

Every stack weight the suite used to load came from synthesize_net: fc_0 sums of
a few thousand to a few ten thousand, PSQT sums of a few thousand.  A real net's
stack weights are whatever training produced, and the evaluated domain is every
net whose stack sums stay inside int32 (PSQT sums wrap mod 2^32 as the oracle's
do).  Two families reach the edges of that domain:

boundary nets   FT weights zero and FT bias 127, so that every valid position
                transforms to x = 126 in every column and
                y[b][o] = b0[b][o] + w0val * 126 * HD exactly: b0 puts a chosen
                target into each (bucket, output) slot.  The same one layer down
                (w1 = 0, or all 30 inputs at 127) for the fc_1 sums z, and for
                fc_2 with all 32 inputs at 127.  psqt_w is uniform in +-2^24, or
                over the whole int32 range in the wrap nets.
extreme nets    the synthetic FT of (seed, HD) kept, every w0, w1, w2 uniform
                int8 over [-128, 127]: full-range MFMA operands at real x.

The bytes of a synthetic net are patched in place, as corpus.edge_net does; the
file layout is the one tests/refpy.py::RefNet parses.  Nothing here uses the
library under test beyond the synthetic net it starts from.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os

import numpy as np

from tests import corpus as Cp
from tests import refpy

L2, L3, FC1_IN, STACKS = 16, 32, 32, 8
X = 126                      # the transformed value of every column of a boundary net
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "golden_stack_domain.json")

# |y| bands of the fc_0 activations: SqrCReLU saturates at 8160; 16384 is the kernel's clamp
# before squaring; 46341^2 leaves int32 and 65536^2 leaves uint32.
BANDS = ((0, 8159), (8160, 16384), (16385, 46340), (46341, 65535), (65536, 1 << 31))
_Y_MAGNITUDES = (1, 63, 64, 65, 724, 725, 8127, 8128, 8129, 8159, 8160, 8191, 8192, 8193, 16383, 16384, 16385,
                 46340, 46341, 65535, 65536, 65537, 1 << 20, 40_000_000)
Y_TARGETS = (0,) + tuple(s * m for m in _Y_MAGNITUDES for s in (1, -1))  # outputs 0..14
# output 15 feeds fwd = y * 9600 / 8128 (C division): y * 9600 leaves int32 at |y| = 223697.
# A net has 8 slots for them (one per bucket): bucket b of a kind takes entry (first + b) % 18, and
# the firsts in KINDS are placed so that the first four kinds hold all 18 and every bucket meets
# both signs (index parity is the sign).
FWD_TARGETS = (1, -1, 8127, -8127, 8128, -8128, 223696, -223696, 223697, -223697, 40_000_000, -40_000_000,
               223698, -223698, 8129, -8129, 1_000_000, -1_000_000)
# fc_1 sums: the CReLU edges of z >> 6, and far out on both sides
Z_TARGETS = (-65, -64, -1, 0, 1, 63, 64, 65, 8127, 8128, 8129, 8191, 8192, 8193, -8192, 1 << 20, -(1 << 20),
             40_000_000, -40_000_000)
Y_SATURATED = (8192, 8193, 16384, 16385, 46340, 46341, 65535, 65536, 65537, 1 << 20, 40_000_000)
Z_SATURATED = (8128, 8129, 8191, 8192, 8193, 1 << 20, 40_000_000)
B2_TARGETS = (2000, -2000, 1 << 20, -(1 << 20))

# kind -> (w0val, rotation of the y targets, first fwd target)
KINDS = {"w0=0": (0, 0, 0), "w0=127": (127, 17, 9), "w0=-128": (-128, 34, 5),
         "fc1_zero": (0, 8, 14), "fc1_sat": (127, 0, 2), "fc2_sat": (-128, 25, 11)}
W0_KINDS = ("w0=0", "w0=127", "w0=-128")
PSQT_24, PSQT_WRAP, PSQT_KEEP = "2^24", "wrap", "keep"
EXTREME_SEEDS = {128: 7, 1024: 1, 1536: 8}
# The numpy seed of every crafted weight.  With one random w0 row per bucket feeding fwd, about
# half the seeds leave some bucket of some extreme net without a negative y15; this one does not
# (test_stack_domain asserts it, with the |y| bands, from refpy).
WEIGHT_SEED = 20240925
NFEAT = {0: refpy.FEATURES, Cp.CRAZYHOUSE: 64 * Cp.VROWS[Cp.CRAZYHOUSE], Cp.ATOMIC: 64 * Cp.VROWS[Cp.ATOMIC]}


def band_of(y) -> np.ndarray:
    a = np.abs(np.asarray(y, dtype=np.int64))
    return np.searchsorted([lo for lo, _ in BANDS], a, side="right") - 1


def _spread(values) -> list[int]:
    """The values ordered so that each band's members lie evenly through the list: any 15
    consecutive entries (cyclically) then hold every band."""
    keyed = []
    for band in range(len(BANDS)):
        mine = [v for v in values if band_of(v) == band]
        keyed += [((i + 0.5) / len(mine) + 1e-3 * band, v) for i, v in enumerate(mine)]
    return [v for _, v in sorted(keyed)]


Y_ORDER = tuple(_spread(Y_TARGETS))


class Image:
    """Writable numpy views of the arrays in a net file's bytes (the layout of refpy.RefNet)."""

    def __init__(self, data: bytes, nfeat: int = refpy.FEATURES):
        self.data = bytearray(data)
        self.nfeat = nfeat
        dlen = int(np.frombuffer(self.data, "<u4", 1, 8)[0])
        fth = int(np.frombuffer(self.data, "<u4", 1, 12 + dlen)[0])
        self.hd = hd = ((fth ^ 0x7F234CB8) & 0xFFFF) // 2  # the variants' hash differs above bit 16
        off = 12 + dlen + 4

        def take(dtype, count):
            nonlocal off
            a = np.frombuffer(self.data, dtype=dtype, count=count, offset=off)
            off += a.nbytes
            return a

        self.ft_bias = take("<i2", hd)
        self.ft_w = take("<i2", nfeat * hd).reshape(nfeat, hd)
        self.psqt = take("<i4", 8 * nfeat).reshape(nfeat, 8)
        self.b0, self.w0, self.b1, self.w1, self.b2, self.w2 = [], [], [], [], [], []
        for _ in range(STACKS):
            off += 4
            self.b0.append(take("<i4", L2))
            self.w0.append(take("i1", L2 * hd).reshape(L2, hd))
            self.b1.append(take("<i4", L3))
            self.w1.append(take("i1", L3 * FC1_IN).reshape(L3, FC1_IN))
            self.b2.append(take("<i4", 1))
            self.w2.append(take("i1", L3))
        assert off == len(self.data), (off, len(self.data))

    def bytes(self) -> bytes:
        return bytes(self.data)


def _base(hd: int, variant: int, seed: int = 1) -> bytes:
    if variant:
        from fishnet_amd import synthesize_variant_net
        return synthesize_variant_net(seed, hd, variant)
    from tests.conftest import net_bytes
    return net_bytes(seed, hd, 0)


def _set_psqt(im: Image, rng, psqt: str) -> None:
    if psqt == PSQT_24:
        im.psqt[:] = rng.integers(-(1 << 24), (1 << 24) + 1, size=im.psqt.shape)
    elif psqt == PSQT_WRAP:
        im.psqt[:] = rng.integers(-(1 << 31), 1 << 31, size=im.psqt.shape)


def y_targets(kind: str) -> np.ndarray:
    """(8, 16) the fc_0 sums a boundary net of this kind gives in every bucket."""
    _, rot, fwd0 = KINDS[kind]
    order = Y_SATURATED if kind == "fc1_sat" else Y_ORDER
    t = np.zeros((STACKS, L2), dtype=np.int64)
    for b in range(STACKS):
        for o in range(L2 - 1):
            t[b, o] = order[(rot + b * (L2 - 1) + o) % len(order)]
        t[b, L2 - 1] = FWD_TARGETS[(fwd0 + b) % len(FWD_TARGETS)]
    return t


def z_targets(kind: str) -> np.ndarray | None:
    """(8, 32) the fc_1 sums of the kinds that fix them (None: fc_1 keeps its synthetic weights)."""
    if kind not in ("fc1_zero", "fc1_sat", "fc2_sat"):
        return None
    order = Z_SATURATED if kind == "fc2_sat" else Z_TARGETS
    rot = 7 if kind == "fc1_sat" else 0
    s = np.arange(STACKS * L3).reshape(STACKS, L3)
    return np.array(order, dtype=np.int64)[(rot + s) % len(order)]


@functools.lru_cache(maxsize=4)
def boundary_net(hd: int, kind: str, psqt: str = PSQT_24, variant: int = 0) -> bytes:
    """One boundary net (module docstring).  kind is a key of KINDS:
    w0=0 / w0=127 / w0=-128   every w0 at that value, y on Y_TARGETS (both signs, every band in
                              every bucket) and FWD_TARGETS; fc_1 and fc_2 stay synthetic
    fc1_zero                  w1 = 0 and b1 on Z_TARGETS, padding weights (inputs 30, 31) at +-127
    fc1_sat                   y >= 8192 in outputs 0..14, so all 30 fc_1 inputs are 127; w1 rows
                              all 127 or all -128, b1 = target - 30 * 127 * w, padding at +-127
    fc2_sat                   w1 = 0 and b1 >= 8128, so all 32 fc_2 inputs are 127; w2 rows all
                              127 or all -128, b2 in +-2000, +-2^20"""
    w0val = KINDS[kind][0]
    im = Image(_base(hd, variant), NFEAT[variant])
    rng = np.random.default_rng([WEIGHT_SEED, hd, list(KINDS).index(kind), variant])
    im.ft_bias[:] = 127
    im.ft_w[:] = 0
    _set_psqt(im, rng, psqt)
    yt, zt = y_targets(kind), z_targets(kind)
    pad = np.where(np.arange(L3) % 2, -127, 127)
    for b in range(STACKS):
        im.w0[b][:] = w0val
        im.b0[b][:] = yt[b] - w0val * X * hd
        im.w2[b][im.w2[b] == 0] = 1  # every fc_1 output reaches the result
        if kind == "fc1_zero":
            im.w1[b][:] = 0
            im.b1[b][:] = zt[b]
        elif kind == "fc1_sat":
            w = np.where((np.arange(L3) + b) % 2, -128, 127)
            im.w1[b][:, :30] = w[:, None]
            im.b1[b][:] = zt[b] - 30 * 127 * w
        elif kind == "fc2_sat":
            im.w1[b][:] = 0
            im.b1[b][:] = zt[b]
            im.w2[b][:] = 127 if b % 2 == 0 else -128
            im.b2[b][0] = B2_TARGETS[b // 2]
        if kind in ("fc1_zero", "fc1_sat"):
            im.w1[b][:, 30] = pad
            im.w1[b][:, 31] = -pad
    return im.bytes()


@functools.lru_cache(maxsize=4)
def extreme_net(hd: int, psqt: str = PSQT_KEEP) -> bytes:
    """The synthetic net of (EXTREME_SEEDS[hd], hd) with every w0, w1 (inputs 0..29) and w2
    uniform over [-128, 127]."""
    im = Image(_base(hd, 0, EXTREME_SEEDS[hd]))
    rng = np.random.default_rng([WEIGHT_SEED, hd, 99])
    _set_psqt(im, rng, psqt)
    for b in range(STACKS):
        im.w0[b][:] = rng.integers(-128, 128, size=im.w0[b].shape)
        im.w1[b][:, :30] = rng.integers(-128, 128, size=(L3, 30))
        im.w2[b][:] = rng.integers(-128, 128, size=L3)
    return im.bytes()


# ---- inputs --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def records() -> np.ndarray:
    """Every 13th corpus record: 517 (32 tiles of 16 and 5 more), at least 39 in every bucket,
    buckets mixed inside the tiles."""
    pos = Cp.chess_corpus()[::13].copy()
    pos.setflags(write=False)
    return pos


def chains(max_positions: int, seed: int = 31) -> tuple[np.ndarray, np.ndarray]:
    """Strip, fill and mixed chains of lengths 3..10 (a segment's deltas go in batches of 8:
    lengths 10 cross into a second batch)."""
    b, stm, _, off = Cp._chains(seed, (Cp.STRIP, Cp.FILL, Cp.MIXED), max_positions, lengths=tuple(range(3, 11)))
    return Cp.pack_boards(b, stm), off


def vchains(variant: int, max_positions: int) -> tuple[np.ndarray, np.ndarray]:
    b, stm, hands, off = Cp._chains(40 + variant, (Cp.STRIP, Cp.FILL, Cp.MIXED), max_positions,
                                    pockets=variant == Cp.CRAZYHOUSE, lengths=tuple(range(3, 11)))
    return Cp.pack_vboards(b, stm, hands), off


# ---- the nets the CPU tests walk -----------------------------------------------------------------

BOUNDARY_HDS = (128, 512, 1024, 1536)  # 3072 holds the w0=-128 net alone
FAMILY = [("boundary", hd, kind, PSQT_24) for hd in BOUNDARY_HDS for kind in KINDS]
FAMILY += [("boundary", 3072, "w0=-128", PSQT_24)]
FAMILY += [("boundary", hd, "w0=0", PSQT_WRAP) for hd in (128, 1024)]
FAMILY += [("extreme", hd, "", PSQT_KEEP) for hd in EXTREME_SEEDS]


def net_id(spec) -> str:
    family, hd, kind, psqt = spec
    return "-".join(str(p) for p in (family, hd, kind, psqt) if p != "")


def make(spec) -> bytes:
    family, hd, kind, psqt = spec
    return boundary_net(hd, kind, psqt) if family == "boundary" else extreme_net(hd, psqt)


def digest(ps: np.ndarray, po: np.ndarray) -> str:
    return hashlib.sha256(ps.astype("<i4").tobytes() + po.astype("<i4").tobytes()).hexdigest()


def main() -> None:
    """Rewrite tests/golden/golden_stack_domain.json from the oracle (after a deliberate change)."""
    from oracle.oracle import OracleNet
    out = {}
    for spec in FAMILY:
        ps, po, rc = OracleNet(make(spec)).eval_packed(records(), threads=8)
        assert rc == 0
        out[net_id(spec)] = digest(ps, po)
    with open(GOLDEN, "w") as f:
        json.dump({"records": "corpus.chess_corpus()[::13]", "sha256": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

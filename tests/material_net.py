"""A net that counts material (test-only, numpy).

The project's nets are random, so "does not hang the queen" cannot be asserted
on them.  This one has every FT weight, FT bias, stack weight and stack bias at
0 and psqt_w[f][*] = +-16 * {100, 300, 300, 500, 900} by the feature's plane
(own piece positive, opponent's piece negative, king planes 0).  Each
perspective's PSQT accumulator is then its material balance times 16, the
evaluation's psqt term the side to move's balance times 16, positional 0, and
s(X) = trunc((psqt + positional) / 16) the material balance in centipawns.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import stack_nets as S

VALUE = {1: 100, 2: 300, 3: 300, 4: 500, 5: 900}  # piece type -> centipawns


@functools.lru_cache(maxsize=2)
def material_net(hd: int = 128) -> bytes:
    im = S.Image(S._base(hd, 0))
    im.ft_bias[:] = 0
    im.ft_w[:] = 0
    for b in range(S.STACKS):
        for a in (im.b0[b], im.w0[b], im.b1[b], im.w1[b], im.b2[b], im.w2[b]):
            a[:] = 0
    plane = (np.arange(im.nfeat) % 704) // 64          # 2 * (type - 1) + (colour != perspective); 10: a king
    value = np.array([VALUE[p // 2 + 1] for p in range(10)] + [0])
    sign = np.where(plane % 2 == 0, 1, -1)
    im.psqt[:] = (16 * value[plane] * np.where(plane == 10, 0, sign))[:, None]
    return im.bytes()


def balance(fen: str) -> int:
    """The side to move's material balance in centipawns, from the FEN's placement alone."""
    board, stm = fen.split()[:2]
    total = 0
    for ch in board:
        t = "pnbrq".find(ch.lower())
        if t >= 0:
            total += VALUE[t + 1] * (1 if ch.isupper() else -1)
    return total if stm == "w" else -total

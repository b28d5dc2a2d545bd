"""The material net for the variants' feature sets (test-only, numpy).

tests/material_net.py for a Fairy-Stockfish variant net: every FT weight, FT
bias, stack weight and stack bias is 0, and psqt_w[f][*] = +-16 * {100, 300,
300, 500, 900} by the feature's plane: a board plane as in material_net.py (own
piece positive, opponent's piece negative, the shared king plane 0), and in a
crazyhouse net a hand row worth its piece, whichever of the 16 copies it is.
s(X) is then the side to move's material balance in centipawns, pieces in hand
included, and positional is 0.

A feature's row inside its king square's block (oracle/variant_oracle.c): rows
0..703 are the 11 board planes of 64 squares, plane = 2 * (type - 1) + (colour
!= perspective), 10 the kings; rows 704.. (crazyhouse) are 10 hand planes of 16
slots in the same order.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import stack_nets as S
from tests.material_net import VALUE

BOARD_ROWS, HAND_SLOTS = 704, 16


@functools.lru_cache(maxsize=4)
def vmaterial_net(hd: int, variant: int) -> bytes:
    nfeat = S.NFEAT[variant]
    im = S.Image(S._base(hd, variant), nfeat)
    im.ft_bias[:] = 0
    im.ft_w[:] = 0
    for b in range(S.STACKS):
        for a in (im.b0[b], im.w0[b], im.b1[b], im.w1[b], im.b2[b], im.w2[b]):
            a[:] = 0
    row = np.arange(nfeat) % (nfeat // 64)
    plane = np.where(row < BOARD_ROWS, row // 64, (row - BOARD_ROWS) // HAND_SLOTS)  # 10: a king (board rows only)
    value = np.array([VALUE[p // 2 + 1] for p in range(10)] + [0])
    sign = np.where(plane % 2 == 0, 1, -1)
    im.psqt[:] = (16 * value[plane] * np.where(plane == 10, 0, sign))[:, None]
    return im.bytes()


def vbalance(fen: str) -> int:
    """The side to move's material balance in centipawns from the FEN's placement and holdings."""
    board, stm = fen.split()[:2]
    total = 0
    for ch in board:
        t = "pnbrq".find(ch.lower())
        if t >= 0 and ch.isalpha():
            total += VALUE[t + 1] * (1 if ch.isupper() else -1)
    return total if stm == "w" else -total

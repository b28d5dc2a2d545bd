"""Deterministic constructed corpora over the whole position domain (test-only).

Every parity test used to take its positions from random play, which reaches
about two thirds of the feature-transformer rows and almost never a board of
one to four pieces.  The kernels accept any record with one king per colour, at
most 32 pieces and stm <= 1, with any piece on any square; the corpora here are
constructed to cover that domain: every reachable FT row, every (perspective,
king block, piece count) bin of the sliced plan, every layer-stack bucket, and
every delta shape of the grouped paths.

Everything is generated in numpy from fixed seeds; no position file is
committed.  Coverage is computed from tests/refpy.py (chess) and from a numpy
restatement of the variant indices (oracle/variant_oracle.c), never with the
library under test.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import refpy

POS_BYTES, VPOS_BYTES = 36, 48
WK, BK = 6, 14
NONKING = (1, 2, 3, 4, 5, 9, 10, 11, 12, 13)
CHESS_ROWS = refpy.FEATURES  # 32 king blocks x 704
CHESS_BINS = 2 * 32 * 31     # perspective x king block x piece count 2..32
CRAZYHOUSE, ATOMIC = 1, 2
VROWS = {CRAZYHOUSE: 704 + 160, ATOMIC: 704}
HAND_MAX = 16                # the largest pocket count a record may carry
MAX_PIECES = 32
# A segment of L plies walks L - 1 deltas in batches of 8; the last batch holds
# (L - 2) % 8 + 1 of them: these lengths put every value 1..8 there, and 31 is
# three full batches plus a last one.
CHAIN_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17, 31)


# ---- records -------------------------------------------------------------------------------------

def pack_boards(boards: np.ndarray, stm: np.ndarray) -> np.ndarray:
    """(n, 64) piece codes + (n,) side to move -> (n, 36) fnnue_pos records."""
    boards = np.asarray(boards, dtype=np.uint8).reshape(-1, 64)
    out = np.zeros((len(boards), POS_BYTES), dtype=np.uint8)
    out[:, :32] = boards[:, 0::2] | (boards[:, 1::2] << 4)
    out[:, 32] = stm
    return out


def pack_vboards(boards: np.ndarray, stm: np.ndarray, hands: np.ndarray | None = None) -> np.ndarray:
    """As pack_boards for fnnue_vpos (48 bytes): hands is (n, 10), white P N B R Q then black."""
    boards = np.asarray(boards, dtype=np.uint8).reshape(-1, 64)
    out = np.zeros((len(boards), VPOS_BYTES), dtype=np.uint8)
    out[:, :32] = boards[:, 0::2] | (boards[:, 1::2] << 4)
    out[:, 32] = stm
    if hands is not None:
        out[:, 33:43] = hands
    return out


def unpack_boards(records: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fnnue_pos or fnnue_vpos records -> ((n, 64) piece codes, (n,) stm)."""
    records = np.asarray(records, dtype=np.uint8)
    records = records.reshape(-1, records.shape[-1])
    boards = np.zeros((len(records), 64), dtype=np.uint8)
    boards[:, 0::2] = records[:, :32] & 15
    boards[:, 1::2] = records[:, :32] >> 4
    return boards, records[:, 32].copy()


def piece_counts(records: np.ndarray) -> np.ndarray:
    return (unpack_boards(records)[0] != 0).sum(axis=1)


def buckets(records: np.ndarray) -> np.ndarray:
    """Layer-stack bucket (pieces on the board - 1) / 4 of every record."""
    return (piece_counts(records) - 1) // 4


def offsets(lengths) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint32)


# ---- board construction --------------------------------------------------------------------------

def _kings(wk: int, bk: int) -> np.ndarray:
    b = np.zeros(64, dtype=np.uint8)
    b[wk], b[bk] = WK, BK
    return b


def _free(board: np.ndarray) -> np.ndarray:
    return np.nonzero(board == 0)[0]


def _scatter(rng, board: np.ndarray, count: int) -> np.ndarray:
    """`count` random non-king pieces on random free squares (any piece on any square)."""
    b = board.copy()
    sq = rng.permutation(_free(b))[:count]
    b[sq] = rng.choice(NONKING, size=len(sq))
    return b


def _sweep_boards() -> list[np.ndarray]:
    """Every king square for each colour (white king on i, black king on 63 - i), every
    non-king piece code on every other square: two boards of 30 identical pieces, and a
    third with the enemy king moved off its square so that square is reached too."""
    out = []
    for i in range(64):
        wk, bk = i, 63 - i
        base = _kings(wk, bk)
        free = _free(base)  # 62 squares
        bk2, wk2 = int(free[(7 * i) % 60]), int(free[(11 * i + 30) % 60])  # where the moved king goes
        for pc in NONKING:
            for chunk in (free[:30], free[30:60]):
                b = base.copy()
                b[chunk] = pc
                out.append(b)
            # the last two free squares and the enemy king's own square, for each colour's view
            b = _kings(wk, bk2)
            b[[free[60], free[61], bk]] = pc
            out.append(b)
            b = _kings(wk2, bk)
            b[[free[60], free[61], wk]] = pc
            out.append(b)
    return out


def _king_pair_boards(rng) -> list[np.ndarray]:
    """Every ordered pair of king squares (each own-king block against the enemy king on each
    of the other 63 squares), the piece count running over 2..32 so that every
    (perspective, king block, count) bin is met from both sides."""
    out = []
    for wk in range(64):
        for bk in range(64):
            if wk != bk:
                out.append(_scatter(rng, _kings(wk, bk), (wk + bk) % 31))
    return out


def _bucket_boards(rng, have: np.ndarray, floor: int) -> list[np.ndarray]:
    """Random boards topping every layer-stack bucket up to `floor` positions; bucket 0 gets
    bare kings, one, and two extra pieces in equal parts."""
    out = []
    for bucket in range(8):
        for j in range(max(0, floor - int(have[bucket]))):
            n = 4 * bucket + 1 + j % 4 if bucket else 2 + j % 3
            sq = rng.permutation(64)[:2]
            out.append(_scatter(rng, _kings(int(sq[0]), int(sq[1])), n - 2))
    return out


@functools.lru_cache(maxsize=1)
def _chess_boards() -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(20240601)
    boards = _sweep_boards() + _king_pair_boards(rng)
    counts = (np.array(boards) != 0).sum(axis=1)
    have = np.bincount((counts - 1) // 4, minlength=8)
    boards += _bucket_boards(rng, have, 520)
    boards = np.array(boards, dtype=np.uint8)
    stm = (np.arange(len(boards)) % 2).astype(np.uint8)  # both sides to move
    stm[rng.random(len(boards)) < 0.25] ^= 1
    boards.setflags(write=False)
    stm.setflags(write=False)
    return boards, stm


def chess_corpus() -> np.ndarray:
    """Packed fnnue_pos records covering the whole chess domain (see the module docstring)."""
    return pack_boards(*_chess_boards())


def sweep_groups(records: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    """The corpus as groups of unrelated boards (consecutive boards differ in far more than
    four squares or in a king square: every step inside a group refreshes)."""
    if records is None:
        records = chess_corpus()
    sizes, n, k = [], 0, 0
    cycle = (1, 2, 3, 5, 8, 9, 17, 31, 64, 0)  # an empty group too
    while n < len(records):
        s = min(cycle[k % len(cycle)], len(records) - n)
        sizes.append(s)
        n += s
        k += 1
    return records, offsets(sizes)


# ---- chains: both kings fixed, so that no perspective refreshes inside a group -------------------

STRIP, FILL, MIXED = "strip", "fill", "mixed"
# (removed, added) squares of one step; a legal move never has the shapes marked *
_MIXED_STEPS = ((1, 0), (0, 1), (0, 2), (2, 0), (1, 2), (0, 0), (1, 1), (2, 1), (2, 2))


def _chain_boards(rng, kind: str, length: int, pockets: bool = False):
    """One chain of `length` boards (and hands).  A strip chain ends on bare kings, a fill
    chain starts from them; with pockets a removed piece may enter the hand (a capture) and an
    added piece may come out of it (a drop), so that board and pocket rows change together."""
    sq = rng.permutation(64)[:2]
    kings = _kings(int(sq[0]), int(sq[1]))
    if kind == STRIP:
        board, steps = _scatter(rng, kings, length - 1), [(1, 0)] * (length - 1)
    elif kind == FILL:
        board, steps = kings, [(0, 1)] * (length - 1)
    else:
        board = _scatter(rng, kings, int(rng.integers(0, 31)))
        steps = [_MIXED_STEPS[int(rng.integers(len(_MIXED_STEPS)))] for _ in range(length - 1)]
    hand = np.zeros(10, dtype=np.uint8)
    if pockets and kind == FILL:
        for _ in range(length - 1):  # a fill chain drops its pieces out of full pockets
            hand[rng.choice(np.nonzero(hand < HAND_MAX)[0])] += 1
    boards, hands = [board.copy()], [hand.copy()]
    for rem, add in steps:
        board = board.copy()
        hand = hand.copy()
        occ = np.nonzero((board != 0) & (board != WK) & (board != BK))[0]
        rem = min(rem, len(occ))
        gone = rng.permutation(occ)[:rem]
        for s in gone:
            pc = int(board[s])
            board[s] = 0
            slot = (pc & 7) - 1 + (0 if pc >> 3 else 5)  # the capturer's pocket
            if pockets and hand[slot] < HAND_MAX and rng.random() < 0.6:
                hand[slot] += 1
        for _ in range(add):
            total = int((board != 0).sum()) + int(hand.sum())
            free = _free(board)
            free = free[~np.isin(free, gone)]  # a square changes once per step
            held = np.nonzero(hand)[0]
            if pockets and len(held) and rng.random() < 0.6 and len(free):
                slot = int(rng.choice(held))  # a drop: out of the hand, onto the board
                hand[slot] -= 1
                board[rng.choice(free)] = slot % 5 + 1 + (8 if slot >= 5 else 0)
            elif total < MAX_PIECES and len(free):
                board[rng.choice(free)] = rng.choice(NONKING)
        boards.append(board.copy())
        hands.append(hand.copy())
    return boards, hands


def _chains(seed: int, kinds, max_positions: int | None, pockets: bool = False, one_king: bool = False,
            lengths=CHAIN_LENGTHS):
    """Chains of every length in CHAIN_LENGTHS for every kind, repeated with new kings and
    pieces until `max_positions` would be passed (one round when it is None)."""
    rng = np.random.default_rng(seed)
    boards, hands, sizes = [], [], []
    while True:
        for kind in kinds:
            for length in lengths:
                if max_positions is not None and len(boards) + length > max_positions:
                    return _finish_chains(rng, boards, hands, sizes, one_king)
                b, h = _chain_boards(rng, kind, length, pockets)
                boards += b
                hands += h
                sizes.append(length)
        if max_positions is None:
            return _finish_chains(rng, boards, hands, sizes, one_king)


def _finish_chains(rng, boards, hands, sizes, one_king):
    boards = np.array(boards, dtype=np.uint8)
    hands = np.array(hands, dtype=np.uint8)
    stm = rng.integers(0, 2, size=len(boards)).astype(np.uint8)
    off = offsets(sizes)
    if one_king:
        # atomic: an exploded king somewhere inside every fourth group of three or more
        for g in range(0, len(sizes), 4):
            if sizes[g] >= 3:
                i = int(off[g]) + 1 + int(rng.integers(sizes[g] - 1))
                boards[i][boards[i] == (WK if g % 8 else BK)] = 0
    return boards, stm, hands, off


def strip_chains(max_positions: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(records, offsets): one piece leaves per ply, down to bare kings; delta shape (1, 0)."""
    b, stm, _, off = _chains(11, (STRIP,), max_positions)
    return pack_boards(b, stm), off


def fill_chains(max_positions: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(records, offsets): one piece enters per ply, up from bare kings; delta shape (0, 1)."""
    b, stm, _, off = _chains(12, (FILL,), max_positions)
    return pack_boards(b, stm), off


def chess_chains(max_positions: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """Strip, fill and mixed chains (steps of shape (0,2) (2,0) (1,2) (0,0) among them) in one
    batch of at most `max_positions` records."""
    b, stm, _, off = _chains(13, (STRIP, FILL, MIXED), max_positions)
    return pack_boards(b, stm), off


def uniform_chains(length: int, max_positions: int) -> tuple[np.ndarray, np.ndarray]:
    """Strip, fill and mixed chains of one length only: every segment of a pass ends together."""
    b, stm, _, off = _chains(100 + length, (STRIP, FILL, MIXED), max_positions, lengths=(length,))
    return pack_boards(b, stm), off


def delta_shapes(records: np.ndarray, off: np.ndarray) -> set[tuple[int, int]]:
    """The (removed, added) square counts of every CHAIN step in the groups."""
    boards, _ = unpack_boards(records)
    shapes = set()
    for g in range(len(off) - 1):
        for i in range(int(off[g]) + 1, int(off[g + 1])):
            a, b = boards[i - 1], boards[i]
            ch = a != b
            shapes.add((int((ch & (a != 0)).sum()), int((ch & (b != 0)).sum())))
    return shapes


# ---- variants ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _variant_boards(variant: int):
    rng = np.random.default_rng(20240700 + variant)
    boards = _sweep_boards() + _king_pair_boards(rng)
    counts = (np.array(boards) != 0).sum(axis=1)
    boards += _bucket_boards(rng, np.bincount((counts - 1) // 4, minlength=8), 100)
    hands = [np.zeros(10, dtype=np.uint8) for _ in boards]
    if variant == CRAZYHOUSE:
        # every hand row of every king block: bare kings, 30 pieces in hand, one slot at its limit
        for i in range(64):
            for slot in range(10):
                h = np.zeros(10, dtype=np.uint8)
                h[slot] = HAND_MAX
                h[(slot + 1 + i % 9) % 10] = MAX_PIECES - 2 - HAND_MAX
                boards.append(_kings(i, 63 - i))
                hands.append(h)
        # every count 0 .. HAND_MAX of every slot, over boards that leave room for it
        for slot in range(10):
            for count in range(HAND_MAX + 1):
                sq = rng.permutation(64)[:2]
                room = MAX_PIECES - 2 - count
                b = _scatter(rng, _kings(int(sq[0]), int(sq[1])), int(rng.integers(0, room + 1)))
                h = np.zeros(10, dtype=np.uint8)
                h[slot] = count
                spare = MAX_PIECES - int((b != 0).sum()) - count
                other = (slot + 3) % 10
                h[other] = min(HAND_MAX, int(rng.integers(0, spare + 1)))
                boards.append(b)
                hands.append(h)
    boards = np.array(boards, dtype=np.uint8)
    hands = np.array(hands, dtype=np.uint8)
    stm = (np.arange(len(boards)) % 2).astype(np.uint8)
    for a in (boards, hands, stm):
        a.setflags(write=False)
    return boards, stm, hands


def variant_corpus(variant: int) -> np.ndarray:
    """Packed fnnue_vpos records for crazyhouse / atomic: all 64 king blocks, every reachable
    board row, every piece count; crazyhouse adds every hand row and pocket count."""
    b, stm, hands = _variant_boards(variant)
    return pack_vboards(b, stm, hands)


def variant_chains(variant: int, max_positions: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """Strip / fill / mixed chains over fnnue_vpos.  Crazyhouse steps move pieces between the
    board and the pockets; atomic groups hold exploded (one-king) records."""
    b, stm, hands, off = _chains(20 + variant, (STRIP, FILL, MIXED), max_positions,
                                 pockets=variant == CRAZYHOUSE, one_king=variant == ATOMIC)
    return pack_vboards(b, stm, hands), off


def one_king(vrecords: np.ndarray) -> np.ndarray:
    """Mask of the records with exactly one king (atomic: exploded)."""
    boards, _ = unpack_boards(vrecords)
    return ((boards == WK).sum(axis=1) + (boards == BK).sum(axis=1)) == 1


# ---- coverage, from the references alone ---------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _chess_index_table() -> np.ndarray:
    """refpy.feature as a table [perspective][king square][piece code][square]."""
    t = np.full((2, 64, 16, 64), -1, dtype=np.int32)
    for persp in range(2):
        for ksq in range(64):
            for pc in NONKING + (WK, BK):
                for sq in range(64):
                    t[persp, ksq, pc, sq] = refpy.feature(persp, sq, pc, ksq)
    return t


def king_block(persp: int, ksq: int) -> int:
    """The 704-row block of perspective persp's features: its own king's feature row / 704."""
    return refpy.feature(persp, ksq, BK if persp else WK, ksq) // 704


def chess_coverage(records: np.ndarray) -> dict:
    """Counts over inputs (not GPU measurements): FT rows touched by either perspective,
    (perspective, king block, piece count) bins hit, positions per layer-stack bucket."""
    boards, _ = unpack_boards(records)
    table = _chess_index_table()
    rows = np.zeros(CHESS_ROWS, dtype=bool)
    bins = np.zeros((2, 32, 33), dtype=bool)
    blocks = np.array([[king_block(p, k) for k in range(64)] for p in range(2)])
    counts = (boards != 0).sum(axis=1)
    n, sq = np.nonzero(boards)
    pc = boards[n, sq]
    for persp, king in ((0, WK), (1, BK)):
        ksq = np.argmax(boards == king, axis=1)
        rows[table[persp, ksq[n], pc, sq]] = True
        bins[persp, blocks[persp][ksq], counts] = True
    return {"positions": len(boards), "rows": rows, "rows_touched": int(rows.sum()),
            "bins_hit": int(bins[:, :, 2:].sum()), "buckets": np.bincount((counts - 1) // 4, minlength=8),
            "counts": np.bincount(counts, minlength=33)}


def chess_unreachable_rows() -> np.ndarray:
    """The rows no record can touch: the own king's square in planes 0..9 of its king block
    (another piece would have to stand on the king)."""
    rows = set()
    for persp in range(2):
        for ksq in range(64):
            for pc in NONKING:
                rows.add(refpy.feature(persp, ksq, pc, ksq))
    return np.array(sorted(rows))


def variant_rows(variant: int, records: np.ndarray, persp: int) -> list[np.ndarray]:
    """Numpy restatement of the variant indices (oracle/variant_oracle.c): per record, the
    feature rows of one perspective (board features, then hand features)."""
    K = VROWS[variant]
    boards, _ = unpack_boards(records)
    flip = 56 if persp else 0
    out = []
    for b, rec in zip(boards, np.asarray(records).reshape(-1, VPOS_BYTES)):
        ksq = int(np.argmax(b == (BK if persp else WK))) ^ flip
        sq = np.nonzero(b)[0]
        pc = b[sq].astype(np.int64)
        typ, col = pc & 7, pc >> 3
        plane = np.where(typ == 6, 10, 2 * (typ - 1) + (col != persp))
        f = [(sq ^ flip) + 64 * plane + K * ksq]
        for slot in range(10):
            owner, pt = slot // 5, slot % 5
            base = 704 + 16 * (2 * pt + (owner != persp)) + K * ksq
            f.append(base + np.arange(int(rec[33 + slot])))
        out.append(np.concatenate(f))
    return out


def variant_coverage(variant: int, records: np.ndarray) -> dict:
    """Counts over inputs: rows of the variant's table touched, piece counts present."""
    K = VROWS[variant]
    rows = np.zeros(64 * K, dtype=bool)
    valid = ~one_king(records)
    for persp in range(2):
        for f in variant_rows(variant, records[valid], persp):
            rows[f] = True
    rec = np.asarray(records).reshape(-1, VPOS_BYTES)
    return {"positions": len(rec), "rows": rows, "rows_touched": int(rows.sum()),
            "counts": np.bincount(piece_counts(rec), minlength=33),
            "buckets": np.bincount(buckets(rec)[valid], minlength=8),
            "hand_counts": [np.unique(rec[:, 33 + s]) for s in range(10)]}


def variant_reachable_rows(variant: int) -> np.ndarray:
    """Derived from the feature set's definition: per king block (64, no mirroring) every
    plane 0..9 square but the own king's, the whole king plane, and 16 rows per pocket plane."""
    K = VROWS[variant]
    ok = np.ones((64, K), dtype=bool)
    for k in range(64):
        ok[k, [64 * plane + k for plane in range(10)]] = False
    return ok.reshape(-1)


# ---- nets ----------------------------------------------------------------------------------------

def edge_net(seed: int, hd: int, mag: tuple[int, int]) -> bytes:
    """A synthetic net whose FT columns each keep one sign over every row with
    |w| in [mag[0], mag[1]] and a zero bias: full-board accumulators reach
    31-32 times mag, close to the doubled-column SWAR limit (2^14).  The first
    half's odd columns stay small (|w| <= 12) so that half the transform pairs
    do not saturate and the evaluation still depends on the position."""
    from tests.conftest import net_bytes
    data = bytearray(net_bytes(seed, hd, 0))
    desc_len = int(np.frombuffer(data, np.uint32, 1, 8)[0])
    o = 12 + desc_len + 4
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(hd) < 0.5, -1, 1)
    w = rng.integers(mag[0], mag[1] + 1, size=(22528, hd)) * sign
    small = np.arange(hd)[1:hd // 2:2]
    w[:, small] = rng.integers(-12, 13, size=(22528, small.size))
    data[o:o + 2 * hd] = bytes(2 * hd)
    data[o + 2 * hd:o + 2 * hd + 2 * 22528 * hd] = w.astype(np.int16).tobytes()
    return bytes(data)


# ---- short legal endgame games (written out; legality is checked by the host builder) ------------

ENDGAMES = [
    # (FEN, UCI moves)
    ("8/8/8/4k3/8/8/3QK3/8 w - - 0 1", "d2d4 e5e6 e2e3 e6f5 d4e4 f5f6 e3f4 f6g7 e4e6 g7h7 f4g5 h7g7 e6e7 g7g8 g5g6 g8h8 e7e8"),
    ("8/8/8/4k3/8/8/3RK3/8 w - - 0 1", "d2d4 e5f5 e2e3 f5e5 e3d3 e5f5 d4e4 f5f6 d3d4 f6f5 d4d5 f5f6 e4e5"),
    ("8/8/8/8/4k3/8/4P3/4K3 w - - 0 1", "e1d2 e4d4 e2e3 d4e4 d2e2 e4d5 e2d3 d5e5 e3e4 e5e6 d3d4 e6d6 e4e5 d6e6 d4e4"),
    ("4k3/8/4K3/4P3/8/8/8/8 w - - 0 1", "e6d6 e8d8 e5e6 d8e8 e6e7 e8f7 d6d7 f7g7 e7e8q g7h6 e8e3 h6h5 e3g3"),
    ("8/8/8/8/4k3/8/1q6/K7 w - - 0 1", "a1b2"),                       # the only move: capture to bare kings
    ("8/8/8/8/8/1k6/8/K1q5 w - - 0 1", ""),                           # mate on the board, no move
    ("k7/2Q5/1K6/8/8/8/8/8 b - - 0 1", ""),                           # stalemate
    ("7k/5K2/6Q1/8/8/8/8/8 w - - 0 1", "g6g7"),                        # mate
    ("8/8/8/8/8/5k2/4p3/4K3 w - - 0 1", "e1d2 f3f2 d2d3 e2e1q d3c4 e1e4 c4b5"),  # black promotes
    ("8/3k4/8/8/8/8/r7/K7 w - - 0 1", "a1a2 d7d6 a2b3"),              # KxR leaves bare kings
    ("8/8/4k3/8/8/3BN3/4K3/8 w - - 0 1", "e3c4 e6d5 c4b6 d5c6 d3e4 c6b6"),  # KBNK, black takes the knight
    ("8/8/8/8/8/2k5/2B5/K6N w - - 0 1", "a1a2 c3c2 h1g3 c2d3 g3f5 d3e4 f5d6"),  # KBNK, black takes the bishop
    ("8/p7/8/8/8/8/P7/K6k w - - 0 1", "a2a4 a7a5 a1b2 h1g2 b2c3 g2f3 c3c4 f3e4 c4b5 e4d5 b5a5 d5c5 a5a6 c5c6 a4a5"),
    ("8/8/8/3pk3/8/3PK3/8/8 w - - 0 1", "d3d4 e5e6 e3f4 e6d6 f4f5 d6c6 f5e5 c6c7 e5d5 c7d7"),
    ("8/8/8/4k3/4p3/8/4P3/4K3 b - - 0 1", "e5d4 e1d2 e4e3 d2e1 d4e4 e1d1 e4f4 d1e1 f4g3 e1f1"),
    ("8/8/1k6/8/8/1K6/1P6/8 w - - 0 1", "b3c4 b6c6 b2b4 c6b6 b4b5 b6b7 c4c5 b7c7 b5b6 c7b7 c5b5 b7b8 b5c6 b8c8 b6b7 c8b8 c6b6"),  # stalemate
    ("8/P7/8/8/8/8/7k/K7 w - - 0 1", "a7a8r h2g3 a8a3 g3f4 a1b2"),   # under-promotion
    ("8/8/8/8/8/k7/p7/K7 b - - 0 1", "a3b3"),                          # then white is stalemated
    ("6k1/8/6K1/8/8/8/8/Q7 w - - 0 1", "a1a8"),                        # KQK mate in one
    ("8/8/8/8/8/2n5/1k6/3K4 w - - 0 1", "d1d2 c3e4 d2e3 e4c5 e3d4 c5b3 d4c4 b3d2 c4d3 b2b3 d3d2"),  # KxN to bare kings
]


def main() -> None:
    """The coverage table of DESIGN.md section 3: the suite's standard inputs against the corpus."""
    import fishnet_amd as F
    from fishnet_amd import nnue

    def row(name, cov, reach=None):
        rows = f"{cov['rows_touched']}" + (f" / {reach}" if reach else "")
        print(f"{name:44s} {cov['positions']:8d}  rows {rows:14s} bins {cov.get('bins_hit', '-')!s:5s} "
              f"buckets {cov['buckets'].tolist()}")

    row("random_playouts(1, 20000)", chess_coverage(F.random_playouts(1, 20000)))
    row("random_playouts(1, 1_000_000)", chess_coverage(F.random_playouts(1, 1_000_000)))
    row("random_playouts(2, 300, PLIES)", chess_coverage(F.random_playouts(2, 300, mode=F.PLAYOUT_PLIES)[0]))
    row("random_playouts(52, 20000, PLIES)", chess_coverage(F.random_playouts(52, 20000, mode=F.PLAYOUT_PLIES)[0]))
    row("chess_corpus()", chess_coverage(chess_corpus()), CHESS_ROWS - len(chess_unreachable_rows()))
    for variant in (CRAZYHOUSE, ATOMIC):
        reach = int(variant_reachable_rows(variant).sum())
        row(f"random_vpositions(3, {variant}, 3000)", variant_coverage(variant, nnue.random_vpositions(3, variant, 3000)), reach)
        row(f"random_vgames(7, {variant}, 400)", variant_coverage(variant, nnue.random_vgames(7, variant, 400)[0]), reach)
        row(f"variant_corpus({variant})", variant_coverage(variant, variant_corpus(variant)), reach)


if __name__ == "__main__":
    main()

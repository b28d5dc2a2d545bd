"""kingOfTheHill and racingKings: the rules csrc/vboard.h adds for the two
variants that share atomic's board-only feature set, on the host
(fnnue_vperft, fnnue_game_end, fnnue_game_vpositions, fnnue_random_vgames) and
the net loader for their ids.

The reference validates every move of such a batch with shakmaty
(`Uci::to_move`, [ref] src/queue.rs:545), which is not available offline.  The
rules are therefore restated here as a small mailbox move generator in pure
Python that shares nothing with vboard.h (bitboards, Kogge-Stone fills): the
library's perft must equal it, and every game the library emits must replay
on it.
"""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import nnue

from .positions import PERFT as CHESS_PERFT, START

KOTH, RK, AT, ZH = N.VARIANT_KINGOFTHEHILL, N.VARIANT_RACINGKINGS, N.VARIANT_ATOMIC, N.VARIANT_CRAZYHOUSE
RK_START = "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1"
P, KN, B, R, Q, K = 1, 2, 3, 4, 5, 6
HILL = {27, 28, 35, 36}  # d4 e4 d5 e5

KNIGHT_D = [(1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2)]
KING_D = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
ROOK_D, BISHOP_D = KING_D[0::2], KING_D[1::2]


def sq(name):
    return (ord(name[1]) - 49) * 8 + ord(name[0]) - 97


class Pos:
    """Mailbox position: b[s] = 0 or colour << 3 | type; cr = set of (colour, rook square)."""

    def __init__(self, variant, b, stm, cr=(), ep=-1):
        self.variant, self.b, self.stm, self.cr, self.ep = variant, list(b), stm, frozenset(cr), ep

    @classmethod
    def from_fen(cls, variant, fen):
        f = fen.split()
        b = [0] * 64
        for r, row in enumerate(f[0].split("/")):
            x = 0
            for ch in row:
                if ch.isdigit():
                    x += int(ch)
                else:
                    b[(7 - r) * 8 + x] = (8 if ch.islower() else 0) | " pnbrqk".index(ch.lower())
                    x += 1
        cr = set()
        for ch in f[2] if len(f) > 2 and f[2] != "-" else "":
            c = 1 if ch.islower() else 0
            cr.add((c, c * 56 + (7 if ch.lower() == "k" else 0)))
        ep = sq(f[3]) if len(f) > 3 and f[3] != "-" else -1
        return cls(variant, b, 0 if f[1] == "w" else 1, cr, ep)

    def king(self, c):
        return self.b.index(c << 3 | K)

    def steps(self, s, deltas, slide):
        """Squares reached from s along deltas (stopping on the first piece, included)."""
        for df, dr in deltas:
            f, r = (s & 7) + df, (s >> 3) + dr
            while 0 <= f < 8 and 0 <= r < 8:
                yield r * 8 + f
                if not slide or self.b[r * 8 + f]:
                    break
                f, r = f + df, r + dr

    def attacked(self, s, by):
        b = self.b
        if any(b[t] == (by << 3 | KN) for t in self.steps(s, KNIGHT_D, False)):
            return True
        if any(b[t] == (by << 3 | K) for t in self.steps(s, KING_D, False)):
            return True
        if any(b[t] in (by << 3 | R, by << 3 | Q) for t in self.steps(s, ROOK_D, True)):
            return True
        if any(b[t] in (by << 3 | B, by << 3 | Q) for t in self.steps(s, BISHOP_D, True)):
            return True
        dr = -1 if by == 0 else 1  # a pawn of `by` attacks s from the rank behind s
        return any(b[t] == (by << 3 | P) for t in self.steps(s, [(-1, dr), (1, dr)], False))

    def over(self):
        """The variant's own end of the game."""
        if self.variant == KOTH:
            return self.king(0) in HILL or self.king(1) in HILL
        if self.variant != RK:
            return False
        wk, bk = self.king(0), self.king(1)
        if wk < 56 and bk < 56:
            return False
        if self.stm == 0 or bk >= 56:
            return True
        # white is home and black to move: on while black's king has a rank-8
        # neighbour free of black pieces that white does not attack
        for t in self.steps(bk, KING_D, False):
            if t >= 56 and not (self.b[t] and self.b[t] >> 3 == 1) and not self.attacked(t, 0):
                return False
        return True

    def play(self, m):
        fr, to, promo, castle = m
        b, us = list(self.b), self.stm
        pc, ep = b[fr], -1
        cr = {x for x in self.cr if x[1] not in (fr, to)}
        if castle:
            rook_from = to
            ks = rook_from > fr
            b[fr] = b[rook_from] = 0
            b[us * 56 + (6 if ks else 2)] = us << 3 | K
            b[us * 56 + (5 if ks else 3)] = us << 3 | R
        else:
            if pc & 7 == P and to == self.ep and (fr & 7) != (to & 7):
                b[to + (-8 if us == 0 else 8)] = 0
            if pc & 7 == P and abs(to - fr) == 16:
                ep = (fr + to) // 2
            b[fr] = 0
            b[to] = (us << 3 | promo) if promo else pc
        if pc & 7 == K:
            cr = {x for x in cr if x[0] != us}
        return Pos(self.variant, b, us ^ 1, cr, ep)

    def pseudo(self):
        b, us = self.b, self.stm
        for s in range(64):
            pc = b[s]
            if not pc or pc >> 3 != us:
                continue
            t = pc & 7
            if t == P:
                up = 8 if us == 0 else -8
                last = 6 if us == 0 else 1
                promos = (Q, R, B, KN) if s >> 3 == last else (0,)
                if not b[s + up]:
                    for p in promos:
                        yield (s, s + up, p, False)
                    if s >> 3 == (1 if us == 0 else 6) and not b[s + 2 * up]:
                        yield (s, s + 2 * up, 0, False)
                for to in self.steps(s, [(-1, 1 if us == 0 else -1), (1, 1 if us == 0 else -1)], False):
                    if (b[to] and b[to] >> 3 != us) or (to == self.ep and not b[to]):
                        for p in promos if b[to] else (0,):
                            yield (s, to, p, False)
                continue
            deltas = {KN: KNIGHT_D, B: BISHOP_D, R: ROOK_D, Q: KING_D, K: KING_D}[t]
            for to in self.steps(s, deltas, t in (B, R, Q)):
                if not b[to] or b[to] >> 3 != us:
                    yield (s, to, 0, False)
        k = self.king(us)
        if k == us * 56 + 4 and not self.attacked(k, us ^ 1):
            for rook, between, path in ((us * 56 + 7, (5, 6), (5, 6)), (us * 56, (1, 2, 3), (3, 2))):
                if (us, rook) in self.cr and b[rook] == (us << 3 | R) and \
                        not any(b[us * 56 + f] for f in between) and \
                        not any(self.attacked(us * 56 + f, us ^ 1) for f in path):
                    yield (k, rook, 0, True)

    def legal(self):
        if self.over():
            return
        us = self.stm
        for m in self.pseudo():
            c = self.play(m)
            if c.attacked(c.king(us), us ^ 1):
                continue
            if self.variant == RK and c.attacked(c.king(us ^ 1), us):
                continue  # racingkings: no move gives check
            yield m, c

    def perft(self, d):
        if d == 0:
            return 1
        return sum(1 if d == 1 else c.perft(d - 1) for _, c in self.legal())

    def key(self):
        return bytes(self.b) + bytes([self.stm])


def vkey(vp):
    b = np.zeros(64, np.uint8)
    b[0::2] = vp[:32] & 15
    b[1::2] = vp[:32] >> 4
    return bytes(b) + bytes([int(vp[32])])


# kingOfTheHill: a king can step onto the hill within the depth; a hill square
# is attacked (the king may not step there); a king already there (over)
KOTH_FENS = [
    "8/8/3k4/8/8/3K4/8/8 w - - 0 1",
    "r3k2r/8/8/8/8/3K4/8/8 w kq - 0 1",
    "8/8/2k5/8/5r2/2K5/8/8 w - - 0 1",
    "rnbq1bnr/pppp1ppp/4k3/4p3/4P3/4K3/PPPP1PPP/RNBQ1BNR w - - 0 1",
]
# racingKings: the catch-up case (white home, black next to rank 8, free and
# attacked squares); both kings reaching rank 8; the only king advance gives
# check (the king leaves the rank between its rook and black's king)
RK_FENS = [
    "8/K6k/8/8/8/8/8/8 w - - 0 1",
    "6K1/k7/8/8/8/8/8/7R b - - 0 1",
    "8/R1K4k/8/8/8/8/8/8 w - - 0 1",
    "8/1K5k/8/8/8/8/8/1Rq5 w - - 0 1",
]


def test_racingkings_start_perft_matches_the_restatement():
    root = Pos.from_fen(RK, RK_START)
    for d in (1, 2, 3):
        assert nnue.vperft(RK, RK_START, d) == root.perft(d), d


@pytest.mark.parametrize("variant,fen", [(KOTH, f) for f in KOTH_FENS] + [(RK, f) for f in RK_FENS])
def test_perft_matches_the_restatement(variant, fen):
    root = Pos.from_fen(variant, fen)
    for d in (1, 2, 3):
        assert nnue.vperft(variant, fen, d) == root.perft(d), (fen, d)


# The published racingKings start counts as recalled (not read from a source).
RK_RECALLED = [21, 421, 11264, 296242, 9472927]


def test_racingkings_start_perft_recalled_counts():
    """Depths 4-5 against the recalled counts, asserted only when the library
    and the restatement both agree with them at depths 1-3 (they do)."""
    root = Pos.from_fen(RK, RK_START)
    lib = [nnue.vperft(RK, RK_START, d) for d in (1, 2, 3)]
    assert lib == [root.perft(d) for d in (1, 2, 3)]
    if lib != RK_RECALLED[:3]:
        pytest.fail(f"recalled counts {RK_RECALLED[:3]} differ from the two implementations' {lib}: see DESIGN.md")
    assert nnue.vperft(RK, RK_START, 4) == RK_RECALLED[3]
    assert nnue.vperft(RK, RK_START, 5) == RK_RECALLED[4]


def test_kingofthehill_start_perft_is_chess_perft():
    counts = dict(CHESS_PERFT)[START]
    for d, want in enumerate(counts, start=1):  # no king reaches the hill in 4 plies
        assert nnue.vperft(KOTH, START, d) == want, d


def err_name(fn, *a):
    with pytest.raises(F.FnnueError) as e:
        fn(*a)
    return e.value.name


def test_kingofthehill_game_end():
    # the white king walks e1-e2-e3-d3-d4
    moves = "e2e4 a7a6 e1e2 a6a5 e2e3 a5a4 e3d3 a4a3 d3d4"
    assert nnue.game_end(START, moves, KOTH) == F.END_NO_MOVES | F.END_VARIANT
    assert nnue.game_end(START, moves.rsplit(" ", 1)[0], KOTH) == 0
    assert err_name(nnue.game_vpositions, KOTH, START, moves + " b7b6") == "FNNUE_E_MOVE"
    assert nnue.vperft(KOTH, "8/8/8/3k4/8/8/8/4K3 w - - 0 1", 1) == 0
    # on the hill and in check: CHECK rides along
    assert nnue.game_end("8/8/8/8/3K3r/8/8/7k w - - 0 1", "", KOTH) == F.END_NO_MOVES | F.END_VARIANT | F.END_CHECK
    # an ordinary mate keeps its flags
    assert nnue.game_end(START, "f2f3 e7e5 g2g4 d8h4", KOTH) == F.END_NO_MOVES | F.END_CHECK


def test_racingkings_game_end_and_legality():
    # white home, black cannot catch up: black (to move) has lost
    assert nnue.game_end("8/K7/8/7k/8/8/8/8 w - - 0 1", "a7a8", RK) == F.END_NO_MOVES | F.END_VARIANT
    # black home alone: white (to move) has lost
    assert nnue.game_end("8/7k/8/K7/8/8/8/8 b - - 0 1", "h7h8", RK) == F.END_NO_MOVES | F.END_VARIANT
    # white home, black next to rank 8 on a free square: the game goes on, and black's catch-up draws
    assert nnue.game_end("8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8", RK) == 0
    assert nnue.game_end("8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8 h7h8", RK) == F.END_NO_MOVES
    # the predicate asks only for a free unattacked rank-8 neighbour
    assert nnue.game_end("K7/7k/8/8/8/8/8/6R1 b - - 0 1", "", RK) == 0  # g8 attacked, h8 free
    assert nnue.game_end("KR6/7k/8/8/8/8/8/8 b - - 0 1", "", RK) == F.END_NO_MOVES | F.END_VARIANT  # both attacked
    assert nnue.game_end("K5n1/7k/8/8/8/8/8/B7 b - - 0 1", "", RK) == F.END_NO_MOVES | F.END_VARIANT  # own piece, attacked
    # black missed the catch-up: the game is decided (white, to move, has won)
    assert nnue.game_end("8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8 h7h6", RK) == F.END_NO_MOVES | F.END_VARIANT
    # a move after the end
    assert err_name(nnue.game_vpositions, RK, "8/K7/8/7k/8/8/8/8 w - - 0 1", "a7a8 h5h6") == "FNNUE_E_MOVE"
    # a checking move
    assert err_name(nnue.game_vpositions, RK, "8/8/8/7k/8/8/8/K5R1 w - - 0 1", "g1h1") == "FNNUE_E_MOVE"
    assert nnue.game_vpositions(RK, "8/8/8/7k/8/8/8/K5R1 w - - 0 1", "g1f1").shape == (2, 48)
    # stalemate is a draw
    assert nnue.game_end("8/8/8/k7/8/8/5q2/7K w - - 0 1", "", RK) == F.END_NO_MOVES
    # pawns and castling rights are refused
    assert err_name(nnue.vpos_from_fen, RK, "8/8/8/8/8/8/krbnNBRK/qrbnNBPQ w - - 0 1") == "FNNUE_E_FEN"
    assert err_name(nnue.game_vpositions, RK, "r3k3/8/8/8/8/8/8/4K3 w q - 0 1", "") == "FNNUE_E_FEN"
    assert nnue.vpos_from_fen(RK, RK_START).shape == (48,)


def test_one_king_positions_are_refused_as_fens():
    for v in (KOTH, RK):
        assert err_name(nnue.vpos_from_fen, v, "8/8/8/8/8/8/8/4K3 w - - 0 1") == "FNNUE_E_FEN"


@pytest.mark.parametrize("variant", [KOTH, RK])
def test_net_loader_accepts_the_new_ids(variant):
    data = F.synthesize_variant_net(7, 256, variant)
    net = F.Net.from_bytes_variant(data, variant)
    assert net.variant == variant
    as_atomic = F.Net.from_bytes_variant(data, AT)  # the same file format and feature set
    assert as_atomic.variant == AT
    assert net.accumulator_bound() == as_atomic.accumulator_bound()
    assert F.Net.from_bytes_variant(F.synthesize_variant_net(7, 256, AT), variant).variant == variant
    zh = F.synthesize_variant_net(7, 256, ZH)
    with pytest.raises(F.FnnueError):
        F.Net.from_bytes_variant(zh, variant)
    with pytest.raises(F.FnnueError) as e:
        F.synthesize_variant_net(7, 256, 5)
    assert e.value.name == "FNNUE_E_ARG"


@pytest.mark.parametrize("variant", [KOTH, RK])
def test_random_games_are_deterministic_and_replay_on_the_restatement(variant):
    pos, off = F.random_vgames(11, variant, 24, 60, threads=3)
    pos2, off2 = F.random_vgames(11, variant, 24, 60, threads=1)
    assert np.array_equal(pos, pos2) and np.array_equal(off, off2)
    one, off1 = F.random_vgames(11, variant, 5, 60, threads=2)  # game i depends on (seed, i) alone
    assert np.array_equal(one, pos[:off[5]]) and np.array_equal(off1, off[:6])
    start = START if variant == KOTH else RK_START
    ended = 0
    for g in range(len(off) - 1):
        cur = Pos.from_fen(variant, start)
        assert vkey(pos[off[g]]) == cur.key()
        for i in range(off[g] + 1, off[g + 1]):
            kids = {c.key(): c for _, c in cur.legal()}
            assert vkey(pos[i]) in kids, (g, i - off[g])
            cur = kids[vkey(pos[i])]


@pytest.mark.parametrize("variant,fen", [(KOTH, "8/8/3k4/8/8/3K4/8/8 w - - 0 1"), (RK, "8/8/K6k/8/8/8/8/2R2r2 w - - 0 1")])
def test_random_games_end_where_the_restatement_ends(variant, fen):
    """Random games from a position near the goal: a game shorter than asked
    for stopped in a position where the restatement has no move either."""
    ended = 0
    for seed in range(24):
        moves = F.random_vgame(seed, variant, fen, 12).split()
        pos = nnue.game_vpositions(variant, fen, moves)
        cur = Pos.from_fen(variant, fen)
        for i in range(1, len(pos)):
            kids = {c.key(): c for _, c in cur.legal()}
            assert vkey(pos[i]) in kids, (seed, i)
            cur = kids[vkey(pos[i])]
        if len(moves) < 12:
            assert not list(cur.legal())
            ended += cur.over()
            assert bool(nnue.game_end(fen, moves, variant) & F.END_VARIANT) == \
                (cur.over() and not (variant == RK and cur.king(0) >= 56 and cur.king(1) >= 56))
    assert ended > 0


def test_random_vpositions_are_valid_records():
    for v in (KOTH, RK):
        pos = F.random_vpositions(3, v, 50, 40)
        assert pos.shape == (50, 48)
        codes = np.concatenate([pos[:, :32] & 15, pos[:, :32] >> 4], axis=1)
        assert ((codes == 6).sum(axis=1) == 1).all() and ((codes == 14).sum(axis=1) == 1).all()
        if v == RK:
            assert not ((codes & 7) == 1).any()  # no pawns

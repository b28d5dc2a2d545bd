"""threeCheck on the host: chess with a counter of remaining checks per colour
(csrc/vboard.h), through fnnue_vperft, fnnue_game_end, fnnue_game_vpositions,
fnnue_random_vgame[s], the FEN counter forms and the net loader for id 5.

As in tests/test_plain_variants.py the rules are restated in pure Python (its
mailbox generator, with the counters added here) and share nothing with
vboard.h: the library's perft must equal the restatement's, and every game the
library emits must replay on it, move by move, to the same end flags.  The
readings of the rules and of the two FEN forms are shakmaty's as recalled
(DESIGN.md §4.5c): nothing on this side pins them to shakmaty itself.
"""
import re

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import nnue

from .positions import PERFT as CHESS_PERFT, START
from .test_plain_variants import Pos, vkey

TC, AT, ZH = N.VARIANT_THREECHECK, N.VARIANT_ATOMIC, N.VARIANT_CRAZYHOUSE
LOST = F.END_NO_MOVES | F.END_VARIANT | F.END_CHECK
WHITE_THIRD = "e2e4 e7e5 d1h5 b8c6 h5f7 e8f7 f1c4 f7e8 c4f7"         # checks on plies 5, 7, 9
BLACK_THIRD = "a2a3 e7e5 a3a4 d8h4 b1c3 h4f2 e1f2 f8c5 f2e1 c5f2"    # checks on plies 6, 8, 10


def read_counters(fields):
    """Remaining checks (white, black) from a FEN's fields: "w+b" right after the en-passant square, or a
    last field "+w+b" of checks given; neither: 3 and 3."""
    if len(fields) > 4 and re.fullmatch(r"[0-3]\+[0-3]", fields[4]):
        return int(fields[4][0]), int(fields[4][2])
    if len(fields) > 4 and re.fullmatch(r"\+[0-3]\+[0-3]", fields[-1]):
        return 3 - int(fields[-1][1]), 3 - int(fields[-1][3])
    return 3, 3


class ThreePos(Pos):
    """tests/test_plain_variants.py's chess position with the counters: left[c] = checks colour c may still give."""

    def __init__(self, b, stm, cr=(), ep=-1, left=(3, 3)):
        super().__init__(TC, b, stm, cr, ep)
        self.left = tuple(left)

    @classmethod
    def from_fen(cls, fen):
        p = Pos.from_fen(TC, fen)
        return cls(p.b, p.stm, p.cr, p.ep, read_counters(fen.split()))

    def over(self):
        return 0 in self.left

    def play(self, m):
        p = Pos.play(self, m)
        left = list(self.left)
        if p.attacked(p.king(p.stm), self.stm):  # the move gave check
            left[self.stm] = max(0, left[self.stm] - 1)
        return ThreePos(p.b, p.stm, p.cr, p.ep, left)

    def flags(self):
        """fnnue_game_end's flags, restated."""
        f = 0 if any(True for _ in self.legal()) else F.END_NO_MOVES
        f |= F.END_CHECK if self.attacked(self.king(self.stm), self.stm ^ 1) else 0
        return f | (F.END_VARIANT if self.over() else 0)


def uci(pos, m):
    fr, to, promo, castle = m
    if castle:
        to = pos.stm * 56 + (6 if to > fr else 2)
    name = lambda s: "abcdefgh"[s & 7] + str((s >> 3) + 1)
    return name(fr) + name(to) + (" pnbrq"[promo] if promo else "")


def replay(fen, moves):
    cur = ThreePos.from_fen(fen)
    for t in moves.split():
        kids = {uci(cur, m): c for m, c in cur.legal()}
        assert t in kids, (fen, moves, t)
        cur = kids[t]
    return cur


def err_name(fn, *a):
    with pytest.raises(F.FnnueError) as e:
        fn(*a)
    return e.value.name


# Low counters with checks available at once: Bb5+ ends the game for white;
# Rd8+ does, and black's Ra1+ is the first of three; Ra1+ is black's last;
# Bxf7+ and Bxf2+ with two left each.
LOW_FENS = [
    "rnbqkbnr/ppp2ppp/8/3pp3/4P3/8/PPPP1PPP/RNBQKBNR w KQkq - 1+1 0 3",
    "4k3/8/8/8/8/8/r2R4/4K3 w - - 1+3 0 1",
    "r3k3/8/8/8/8/8/8/4K2R b K - 3+1 0 1",
    "r1bqk2r/pppp1ppp/2n2n2/2b1p3/2B1P3/2N2N2/PPPP1PPP/R1BQK2R w KQkq - 2+2 4 5",
]


@pytest.mark.parametrize("fen", [START] + LOW_FENS)
def test_perft_matches_the_restatement(fen):
    root = ThreePos.from_fen(fen)
    counts = [root.perft(d) for d in (1, 2, 3)]
    assert [nnue.vperft(TC, fen, d) for d in (1, 2, 3)] == counts, fen
    if 1 in root.left:  # a last check within two plies ends its line: chess counts more
        assert counts[2] < Pos.from_fen(TC, fen).perft(3), fen


def test_perft_is_chess_perft_up_to_depth_5():
    """With 3+3 a side moves at most three times within five plies, and a leaf's own end is not counted."""
    for fen, counts in CHESS_PERFT:
        for d, want in enumerate(counts, start=1):
            if d <= 5:
                assert nnue.vperft(TC, fen, d) == want, (fen, d)
                assert nnue.vperft(TC, fen + " +0+0" if len(fen.split()) == 6 else fen, d) == want


def test_named_games_on_the_restatement_and_the_library():
    for moves, winner in ((WHITE_THIRD, 0), (BLACK_THIRD, 1)):
        last = replay(START, moves)
        assert last.left[winner] == 0 and last.left[winner ^ 1] == 3 and last.stm == winner ^ 1
        assert last.flags() == LOST and not list(last.legal())
        before = replay(START, moves.rsplit(" ", 1)[0])
        assert before.left[winner] == 1 and before.flags() == 0
        assert nnue.game_end(START, moves, TC) == LOST
        assert nnue.game_end(START, moves.rsplit(" ", 1)[0], TC) == 0
        n = len(moves.split())
        assert nnue.game_vpositions(TC, START, moves).shape == (n + 1, 48)
        for extra in ("a7a6", "h2h3", "e8f7", "e1f2"):
            with pytest.raises(F.FnnueError) as e:
                nnue.game_vpositions(TC, START, moves + " " + extra)
            assert e.value.name == "FNNUE_E_MOVE" and f"ply {n + 1}" in str(e.value)
        assert nnue.vperft(TC, START, 1) == 20
    # the same moves are no end of a chess-rules variant game, and the records carry no counters
    assert nnue.game_end(START, WHITE_THIRD, N.VARIANT_KINGOFTHEHILL) == F.END_CHECK
    assert np.array_equal(nnue.game_vpositions(TC, START, WHITE_THIRD),
                          nnue.game_vpositions(N.VARIANT_KINGOFTHEHILL, START, WHITE_THIRD))


def test_checkmate_by_the_third_check():
    # Qh4 is mate and black's last check; with a check to spare it is a plain mate
    fool = "f2f3 e7e5 g2g4 d8h4"
    assert nnue.game_end(START[:-3] + "3+1 0 1", fool, TC) == LOST
    assert nnue.game_end(START, fool, TC) == F.END_NO_MOVES | F.END_CHECK
    assert replay(START[:-3] + "3+1 0 1", fool).flags() == LOST
    # stalemate keeps its flags
    assert nnue.game_end("7k/5Q2/8/8/8/8/8/K7 b - - 3+3 0 1", "", TC) == F.END_NO_MOVES


def test_fen_counter_forms():
    base = "r1bqk2r/pppp1ppp/2n2n2/2b1p3/2B1P3/2N2N2/PPPP1PPP/R1BQK2R w KQkq -"
    a, b = base + " 1+3 4 5", base + " 4 5 +2+0"
    assert np.array_equal(nnue.vpos_from_fen(TC, a), nnue.vpos_from_fen(TC, b))
    assert np.array_equal(nnue.vpos_from_fen(TC, a), nnue.vpos_from_fen(TC, base + " 4 5"))
    for d in (1, 2, 3):
        assert nnue.vperft(TC, a, d) == nnue.vperft(TC, b, d) == ThreePos.from_fen(a).perft(d)
    assert nnue.vperft(TC, a, 3) < nnue.vperft(TC, base + " 4 5", 3)  # 3+3: Bxf7+ is not the end
    assert nnue.vperft(TC, base, 3) == nnue.vperft(TC, base + " 3+3 4 5", 3) == nnue.vperft(TC, base + " 4 5 +0+0", 3)
    # a 2+3 root: the first named game ends with white's second check, on ply 7
    seven = " ".join(WHITE_THIRD.split()[:7])
    for root in (START[:-3] + "2+3 0 1", START + " +1+0"):
        assert nnue.game_end(root, seven, TC) == LOST
        assert nnue.game_end(root, " ".join(seven.split()[:6]), TC) == 0
        assert err_name(nnue.game_vpositions, TC, root, seven + " f7e8") == "FNNUE_E_MOVE"
    assert nnue.game_end(START, seven, TC) == F.END_CHECK
    # refused: both forms, digits outside 0..3, malformed fields, both counters 0
    for tail in ("2+3 0 1 +1+0", "4+3 0 1", "3+4 0 1", "0 1 +4+0", "0 1 +0+4", "3+ 0 1", "+3 0 1", "3+3+3 0 1",
                 "0 1 +1", "0 1 +1+0+2", "a+3 0 1", "0 1 +a+0", "0+0 0 1", "0 1 +3+3", "0 +1+0 1", "3-3 0 1 +0"):
        for fn, args in ((nnue.vpos_from_fen, ()), (nnue.game_vpositions, ("",)), (nnue.vperft, (1,))):
            with pytest.raises(F.FnnueError) as e:
                fn(TC, START[:-3] + tail, *args)
            assert e.value.name == "FNNUE_E_FEN", tail
    # the other variants read no counters: their FENs are what they were
    assert nnue.vpos_from_fen(N.VARIANT_KINGOFTHEHILL, START[:-3] + "4+3 0 1").shape == (48,)


def test_root_with_a_zero_counter_is_over():
    # the side to move's own counter is 0: it has already won (the racingkings precedent)
    for fen in ("4k3/8/8/8/8/8/8/4K2R w K - 0+2 0 1", "4k3/8/8/8/8/8/8/4K2R b K - 2+0 0 1",
                "4k3/8/8/8/8/8/8/4K2R w K - 0 1 +3+1"):
        assert nnue.game_end(fen, "", TC) == F.END_NO_MOVES | F.END_VARIANT
        assert nnue.vperft(TC, fen, 1) == 0
        assert err_name(nnue.game_vpositions, TC, fen, "e1e2" if " w " in fen else "e8e7") == "FNNUE_E_MOVE"
        assert ThreePos.from_fen(fen).flags() == F.END_NO_MOVES | F.END_VARIANT
    # the other side's counter is 0: the side to move has lost, in check or not
    assert nnue.game_end("4k3/8/8/8/8/8/8/4K2R w K - 2+0 0 1", "", TC) == F.END_NO_MOVES | F.END_VARIANT
    assert nnue.game_end("4k3/8/8/8/8/8/8/r3K3 w - - 2+0 0 1", "", TC) == LOST


def test_net_loader_and_abi():
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 8
    assert N.lib.fnnue_abi_version() >> 16 == 3
    assert TC == 5 and F.VARIANT_THREECHECK == 5
    data = F.synthesize_variant_net(7, 256, AT)
    net = F.Net.from_bytes_variant(data, TC)
    assert net.variant == TC
    assert net.accumulator_bound() == F.Net.from_bytes_variant(data, AT).accumulator_bound()
    with pytest.raises(F.FnnueError):
        F.Net.from_bytes_variant(F.synthesize_variant_net(7, 256, ZH), TC)
    with pytest.raises(F.FnnueError) as e:
        F.Net.from_bytes_variant(data, 6)
    assert e.value.name == "FNNUE_E_ARG"
    assert err_name(nnue.vperft, 6, START, 1) == "FNNUE_E_ARG"


def test_random_games_replay_on_the_restatement_with_the_same_end_flags():
    """Games of fnnue_random_vgames(5, ...) position by position, and the same walk as move text
    (fnnue_random_vgame) to fnnue_game_end's flags; at least one game ends by the third check."""
    pos, off = F.random_vgames(11, TC, 40, 120, threads=3)
    pos2, off2 = F.random_vgames(11, TC, 40, 120, threads=1)
    assert np.array_equal(pos, pos2) and np.array_equal(off, off2)
    by_rule = 0
    for g in range(len(off) - 1):
        cur, moves = ThreePos.from_fen(START), []
        assert vkey(pos[off[g]]) == cur.key()
        for i in range(off[g] + 1, off[g + 1]):
            kids = {c.key(): (m, c) for m, c in cur.legal()}
            assert vkey(pos[i]) in kids, (g, i - off[g])
            m, nxt = kids[vkey(pos[i])]
            moves.append(uci(cur, m))
            cur = nxt
        flags = cur.flags()
        assert nnue.game_end(START, moves, TC) == flags, (g, moves)
        if flags & F.END_VARIANT:
            assert flags == LOST and 0 in cur.left
            by_rule += 1
    assert by_rule >= 1
    for seed in range(6):  # from a root with one check left each: most games end by the rule at once
        fen = LOW_FENS[3].replace("2+2", "1+1")
        moves = F.random_vgame(seed, TC, fen, 40)
        last = replay(fen, moves)
        assert nnue.game_end(fen, moves, TC) == last.flags()
        assert len(moves.split()) == 40 or last.flags() & F.END_NO_MOVES


def test_random_vpositions_are_valid_records():
    pos = F.random_vpositions(3, TC, 50, 40)
    assert pos.shape == (50, 48)
    codes = np.concatenate([pos[:, :32] & 15, pos[:, :32] >> 4], axis=1)
    assert ((codes == 6).sum(axis=1) == 1).all() and ((codes == 14).sum(axis=1) == 1).all()
    assert not pos[:, 33:43].any()  # empty pockets

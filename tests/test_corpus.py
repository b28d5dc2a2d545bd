"""The constructed corpora (tests/corpus.py) on the CPU: the coverage they must
have, computed from the references alone; the three restatements (scalar
oracle, SIMD baseline, tests/refpy.py) agreeing on them, from scratch and in
CHAIN / STAR groups; the host library where it runs without a GPU; and a golden
digest of the oracle's outputs on this domain.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle import oracle as O
from tests import corpus as Cp
from tests import refpy
from tests.conftest import net_bytes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "golden_corpus_evals.json")
NETS = [(1, 1024, 0), (3, 1024, N.SYNTH_WRAP), (7, 128, 0)]
ZH, AT = Cp.CRAZYHOUSE, Cp.ATOMIC


@pytest.fixture(scope="module")
def corpus():
    pos = Cp.chess_corpus()
    pos.setflags(write=False)
    return pos


@pytest.fixture(scope="module")
def chains():
    """Every chain the GPU tests run, as one batch of groups."""
    parts = [Cp.strip_chains(), Cp.fill_chains(), Cp.chess_chains(2048), Cp.chess_chains(2600)]
    pos = np.concatenate([p for p, _ in parts])
    sizes = np.concatenate([np.diff(o.astype(np.int64)) for _, o in parts])
    return pos, Cp.offsets(sizes)


# ---- coverage conditions -----------------------------------------------------------------------

def test_chess_corpus_covers_every_reachable_row_bin_and_bucket(corpus):
    cov = Cp.chess_coverage(corpus)
    unreachable = Cp.chess_unreachable_rows()
    assert len(unreachable) == 320 and Cp.CHESS_ROWS - 320 == 22208
    assert cov["rows_touched"] == 22208
    assert np.array_equal(np.nonzero(~cov["rows"])[0], unreachable)  # exactly the own-king-square rows
    assert Cp.CHESS_BINS == 1984 and cov["bins_hit"] == 1984
    assert cov["buckets"].min() >= 500, cov["buckets"]
    assert cov["counts"][2] > 0 and cov["counts"][32] > 0 and np.all(cov["counts"][2:] > 0)
    assert cov["counts"][:2].sum() == 0 and len(cov["counts"]) == 33
    assert 5000 < len(corpus) < 16000
    boards, stm = Cp.unpack_boards(corpus)
    assert set(np.unique(stm)) == {0, 1}
    assert set(np.unique(stm[Cp.buckets(corpus) == 0])) == {0, 1}
    for rank in (0, 7):  # pawns on ranks 1 and 8, either colour
        for pawn in (1, 9):
            assert (boards[:, 8 * rank:8 * rank + 8] == pawn).any()
    assert ((boards == 5).sum(axis=1).max(), (boards == 13).sum(axis=1).max()) == (30, 30)  # far beyond legal play
    kings = {(int(np.argmax(b == Cp.WK)), int(np.argmax(b == Cp.BK))) for b in boards}
    assert len(kings) == 64 * 63  # every ordered pair of king squares


def test_coverage_function_is_refpy_feature(corpus):
    """chess_coverage's table is refpy.feature: rows recomputed record by record on a sample."""
    sample = corpus[::97]
    rows = set()
    for rec in sample:
        board, _ = O.unpack(rec)
        wk, bk = int(np.argmax(board == Cp.WK)), int(np.argmax(board == Cp.BK))
        for persp, ksq in ((0, wk), (1, bk)):
            got = sorted(refpy.feature(persp, s, int(pc), ksq) for s, pc in enumerate(board) if pc)
            assert got == O.features(board, persp)  # and the oracle's
            rows.update(got)
    assert set(np.nonzero(Cp.chess_coverage(sample)["rows"])[0].tolist()) == rows


def test_chains_have_every_delta_shape_and_length(chains):
    pos, off = Cp.strip_chains()
    assert Cp.delta_shapes(pos, off) == {(1, 0)}
    sizes = np.diff(off.astype(np.int64)).tolist()
    assert sizes == list(Cp.CHAIN_LENGTHS) and {1, 2, 8, 9, 10, 16, 17, 31} <= set(sizes)
    assert {(s - 2) % 8 + 1 for s in sizes if s > 1} == set(range(1, 9))  # deltas in a segment's last batch of 8
    for length in (2, 5, 31):
        p, o = Cp.uniform_chains(length, 400)
        assert set(np.diff(o.astype(np.int64)).tolist()) == {length} and 400 - length < len(p) <= 400
    counts = Cp.piece_counts(pos)
    assert counts[off[-2]] == 32 and all(counts[o - 1] == 2 for o in off[1:])  # 32 pieces down to bare kings
    assert np.array_equal(Cp.buckets(pos[off[-2]:off[-1]]), (np.arange(32, 1, -1) - 1) // 4)  # 7 -> 0
    pos, off = Cp.fill_chains()
    assert Cp.delta_shapes(pos, off) == {(0, 1)}
    counts = Cp.piece_counts(pos)
    assert counts[off[-1] - 1] == 32 and all(counts[o] == 2 for o in off[:-1])
    small, large = Cp.chess_chains(2048), Cp.chess_chains(2600)
    assert 1800 < len(small[0]) <= 2048 < len(large[0])  # the one-workgroup plan and the kernel chain
    for p, o in (small, large):
        shapes = Cp.delta_shapes(p, o)
        assert {(1, 0), (0, 1), (0, 2), (2, 0), (1, 2), (0, 0), (1, 1), (2, 1), (2, 2)} <= shapes
        assert max(a for a, _ in shapes) <= 2 and max(b for _, b in shapes) <= 2
        assert set(np.diff(o.astype(np.int64)).tolist()) == set(Cp.CHAIN_LENGTHS)
        boards, _ = Cp.unpack_boards(p)
        for g in range(len(o) - 1):  # both kings fixed inside every group
            grp = boards[o[g]:o[g + 1]]
            assert (np.argmax(grp == Cp.WK, axis=1) == np.argmax(grp[0] == Cp.WK)).all()
            assert (np.argmax(grp == Cp.BK, axis=1) == np.argmax(grp[0] == Cp.BK)).all()
        assert np.bincount(Cp.buckets(p), minlength=8).min() > 50
    pos, off = chains
    assert off[-1] == len(pos)


def test_sweep_groups_refresh_at_every_step(corpus):
    pos, off = Cp.sweep_groups()
    assert off[-1] == len(pos) == len(corpus) and 0 in np.diff(off.astype(np.int64))
    boards, _ = Cp.unpack_boards(pos)
    changed = (boards[1:] != boards[:-1]).sum(axis=1)
    moved = (np.argmax(boards[1:] == Cp.WK, axis=1) != np.argmax(boards[:-1] == Cp.WK, axis=1)) & \
            (np.argmax(boards[1:] == Cp.BK, axis=1) != np.argmax(boards[:-1] == Cp.BK, axis=1))
    inside = np.ones(len(pos) - 1, dtype=bool)
    inside[off[1:-1][off[1:-1] > 0] - 1] = False  # steps across a group boundary do not count
    assert ((changed > 4) | moved)[inside].mean() > 0.95


@pytest.mark.parametrize("variant", [ZH, AT])
def test_variant_corpus_covers_its_table(variant):
    pos = Cp.variant_corpus(variant)
    cov = Cp.variant_coverage(variant, pos)
    reach = Cp.variant_reachable_rows(variant)
    # derived here from the feature set's definition, not read from the library
    per_block = 10 * 63 + 64 + (10 * 16 if variant == ZH else 0)
    assert int(reach.sum()) == 64 * per_block and len(reach) == 64 * Cp.VROWS[variant]
    assert np.array_equal(cov["rows"], reach)
    assert np.all(cov["counts"][2:] > 0) and cov["counts"][:2].sum() == 0
    assert cov["buckets"].min() >= 100
    boards, stm = Cp.unpack_boards(pos)
    assert {int(np.argmax(b == Cp.WK)) for b in boards} == set(range(64))
    assert {int(np.argmax(b == Cp.BK)) for b in boards} == set(range(64))
    hands = pos[:, 33:43]
    total = Cp.piece_counts(pos) + hands.sum(axis=1)
    assert total.max() == 32 and hands.max() == (Cp.HAND_MAX if variant == ZH else 0)
    if variant == ZH:
        for slot in range(10):  # every count the record format allows: 0 .. 16 (2 + 16 <= 32)
            assert cov["hand_counts"][slot].tolist() == list(range(Cp.HAND_MAX + 1))
        assert ((Cp.piece_counts(pos) == 2) & (hands.sum(axis=1) == 30)).sum() >= 640
    # the numpy restatement of the indices is the oracle's
    for i in range(0, len(pos), 53):
        for persp in range(2):
            assert sorted(Cp.variant_rows(variant, pos[i:i + 1], persp)[0].tolist()) == \
                O.variant_features(variant, pos[i], persp)


@pytest.mark.parametrize("variant", [ZH, AT])
def test_variant_chains(variant):
    small, large = Cp.variant_chains(variant, 2048), Cp.variant_chains(variant, 2600)
    assert len(small[0]) <= 2048 < len(large[0])
    for pos, off in (small, large):
        gone = Cp.one_king(pos)
        assert (gone.sum() > 5) == (variant == AT)
        assert not gone[off[:-1]].any()  # inside groups, never a group's first record
        hands = pos[:, 33:43].astype(np.int64)
        total = Cp.piece_counts(pos) + hands.sum(axis=1)
        assert total.max() <= 32 and hands.max() <= Cp.HAND_MAX
        if variant == ZH:  # pockets and board change in the same step
            boards, _ = Cp.unpack_boards(pos)
            both = ((boards[1:] != boards[:-1]).any(axis=1)) & ((hands[1:] != hands[:-1]).any(axis=1))
            assert both.sum() > 300
        else:
            assert hands.max() == 0


# ---- the references agree ------------------------------------------------------------------------

def _same(a, b):
    return a[2] == b[2] == 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("seed,hd,flags", NETS)
def test_references_agree_on_corpus_and_chains(corpus, chains, seed, hd, flags):
    """Scalar oracle == SIMD baseline (AVX2, and AVX-512 where the host has it) from scratch
    and along CHAIN / STAR groups; both == refpy on a fixed sample holding every bucket; and
    the golden digest of the oracle's outputs on the corpus."""
    data = net_bytes(seed, hd, flags)
    on = O.OracleNet(data)
    gpos, goff = chains
    spos, soff = Cp.sweep_groups(corpus)
    want, gwant = on.eval_packed(corpus, threads=4), on.eval_packed(gpos, threads=4)
    assert want[2] == 0 and gwant[2] == 0
    try:
        for isa in (0, 1):
            if O.lib.cpu_simd_set_isa(isa) != isa:
                continue  # no AVX-512 VNNI here: AVX2 has run
            assert _same(want, on.simd_eval_packed(corpus, threads=4))
            for mode in (N.GROUP_CHAIN, N.GROUP_STAR):
                assert _same(gwant, on.simd_eval_groups(gpos, goff, mode, threads=4)), (isa, mode)
                assert _same(want, on.simd_eval_groups(spos, soff, mode, threads=4)), (isa, mode)
    finally:
        O.lib.cpu_simd_set_isa(1)
    rn = refpy.RefNet(data)
    b = Cp.buckets(corpus)
    sample = np.concatenate([np.nonzero(b == k)[0][:40] for k in range(8)] +
                            [np.nonzero(Cp.piece_counts(corpus) == 2)[0][:8]])
    assert len(sample) >= 300 and set(b[sample]) == set(range(8))
    for i in sample:
        board, stm = O.unpack(corpus[i])
        assert refpy.evaluate(rn, board, stm) == (int(want[0][i]), int(want[1][i])), i
    bare = Cp.piece_counts(corpus) == 2
    assert np.unique(want[1][bare]).size > 20  # bucket 0 answers depend on the position
    golden = {(e["seed"], e["hd"], e["flags"]): e for e in json.load(open(GOLDEN))["nets"]}
    entry = golden[(seed, hd, flags)]
    assert entry["positions"] == len(corpus) and entry["chain_positions"] == len(gpos)
    assert _digest(want) == entry["corpus_sha256"] and _digest(gwant) == entry["chains_sha256"]
    assert hashlib.sha256(corpus.tobytes()).hexdigest() == json.load(open(GOLDEN))["corpus_records_sha256"]


def _digest(res):
    return hashlib.sha256(res[0].astype("<i4").tobytes() + res[1].astype("<i4").tobytes()).hexdigest()


@pytest.mark.parametrize("variant,hd", [(ZH, 256), (AT, 256), (ZH, 1024)])
def test_variant_oracle_grouped_equals_from_scratch(variant, hd):
    on = O.VariantOracleNet(F.synthesize_variant_net(5, hd, variant), variant)
    golden = json.load(open(GOLDEN))["variants"]
    pos = Cp.variant_corpus(variant)
    want = on.eval_packed(pos, threads=4)
    assert want[2] == 0
    assert _digest(want) == golden[f"{variant}:{hd}"]
    off = Cp.sweep_groups(pos)[1]
    for mode in (N.GROUP_CHAIN, N.GROUP_STAR):
        assert _same(want, on.eval_groups(pos, off, mode))
    gpos, goff = Cp.variant_chains(variant, 2600)
    gwant = on.eval_packed(gpos, threads=4)
    assert gwant[2] == 0
    gone = Cp.one_king(gpos)
    assert np.all(gwant[0][gone] == 0) and np.all(gwant[1][gone] == 0)  # exploded: (0, 0), no error
    assert np.unique(gwant[1][~gone]).size > 1000
    for mode in (N.GROUP_CHAIN, N.GROUP_STAR):
        assert _same(gwant, on.eval_groups(gpos, goff, mode))


# ---- the host library, no GPU --------------------------------------------------------------------

def test_packing_helpers_round_trip(corpus):
    boards, stm = Cp.unpack_boards(corpus)
    assert np.array_equal(Cp.pack_boards(boards, stm), corpus)
    for i in range(0, len(corpus), 331):
        b, s = O.unpack(corpus[i])
        assert np.array_equal(b, boards[i]) and s == stm[i] and np.array_equal(O.pack(b, s), corpus[i])
    assert np.array_equal(F.pos_from_fen("4k3/8/8/8/8/8/8/4K3 w - - 0 1"),
                          Cp.pack_boards(Cp._kings(4, 60), np.array([0]))[0])


def test_accumulator_bound_holds_on_the_corpus(corpus):
    """Net.accumulator_bound() bounds every accumulator column of every record the kernels
    accept, 30 identical pieces included (the oracle's trace gives the accumulators)."""
    data = Cp.edge_net(21, 256, (400, 500))
    net = F.Net.from_bytes(data)
    bound = net.accumulator_bound()
    assert 31 * 400 * 2 < bound < 32768 and int(net.slice_bounds().max()) == bound
    on = O.OracleNet(data)
    full = np.nonzero(Cp.piece_counts(corpus) == 32)[0]
    assert len(full) > 1000
    worst, half = 0, 256 // 2
    for i in full[::7]:
        board, stm = O.unpack(corpus[i])
        acc = on.trace(board, stm)[3].astype(np.int64).reshape(2, 256)
        worst = max(worst, int(np.abs(acc[:, :half]).max()), int(2 * np.abs(acc[:, half:]).max()))
    assert 0.8 * bound < worst <= bound  # far closer to the bound than playouts come


def test_endgame_games_replay_on_the_host():
    """The written-out endgame games are legal (the host builder replays them), reach bucket 0
    on every ply, and hold a capture to bare kings, a promotion, a mate and a stalemate."""
    assert len(Cp.ENDGAMES) >= 20
    ends, bare, promoted = [], 0, 0
    for fen, moves in Cp.ENDGAMES:
        pos = F.game_positions(fen, moves)
        assert len(pos) == len(moves.split()) + 1
        assert Cp.piece_counts(pos).max() <= 4 and (Cp.buckets(pos) == 0).all()
        bare += int(Cp.piece_counts(pos)[-1] == 2)
        promoted += any(len(m) == 5 for m in moves.split())
        ends.append(F.game_end(fen, moves))
        kids, off = F.game_children(fen, moves)
        assert len(off) == len(pos) + 1 and np.array_equal(kids[off[:-1]], pos)
        kb = Cp.unpack_boards(kids)[0]  # no child takes a king: the side not to move is never in check
        assert ((kb == Cp.WK).sum(axis=1) == 1).all() and ((kb == Cp.BK).sum(axis=1) == 1).all()
    assert bare >= 3 and promoted >= 3
    assert ends.count(F.END_NO_MOVES | F.END_CHECK) >= 3 and ends.count(F.END_NO_MOVES) >= 3

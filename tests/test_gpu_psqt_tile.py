"""The bucket-major PSQT tile of ft_slices (DESIGN.md §4.2 "PSQT tile",
fishnet_amd/csrc/psqt_tile.h) on the GPU: psqt and positional bit-exact against
the CPU oracle through fnnue_eval_positions_device with the sliced feature
transformer forced.

Inputs: random playouts of 0-160 plies (2..32 pieces, all eight buckets) and
hand-made positions: for several king placements (several king blocks, so
units and own-king rows differ) every piece count from 2 (kings only: one list
entry, the rest padding) to 32, so that consecutive items of a king block
straddle every bucket boundary (4/5, 8/9, ... 28/29) inside one pass.  Nets:
HD 128 (two slices) and HD 1024, SWAR on, off and a mixed mask (the three
kernel instantiations); crazyhouse at HD 256 with pockets filled (the hand
rows of the 864-row geometry) and atomic at HD 256.  The synthetic nets' PSQT
weights differ per (row, bucket), so a transposition slip cannot cancel."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from oracle.oracle import OracleNet, VariantOracleNet

pytestmark = pytest.mark.gpu

CZH, ATOMIC = F.VARIANT_CRAZYHOUSE, F.VARIANT_ATOMIC
# (white king, black king) squares, a1 = 0: different king blocks for both perspectives
KINGS = [(4, 60), (0, 63), (7, 56), (27, 36), (22, 41)]
ORDER = "PpNnBbRrQqPpPpNnBbRrPpPpPpPpPp"  # the 30 pieces added after the kings, colours alternating


def fen_of(board: dict, stm: str, pocket: str = "") -> str:
    ranks = []
    for r in range(7, -1, -1):
        row, gap = "", 0
        for f in range(8):
            pc = board.get(8 * r + f)
            if pc is None:
                gap += 1
            else:
                row += (str(gap) if gap else "") + pc
                gap = 0
        ranks.append(row + (str(gap) if gap else ""))
    return "/".join(ranks) + (f"[{pocket}]" if pocket else "") + f" {stm} - - 0 1"


def ladder_boards():
    """For every king placement, boards of 2, 3, ... 32 pieces (each adds one piece to the last)."""
    out = []
    for k, (wk, bk) in enumerate(KINGS):
        board = {wk: "K", bk: "k"}
        free = [s for s in range(8, 56) if s not in board]  # pawns stay off the back ranks
        rng = np.random.default_rng(100 + k)
        rng.shuffle(free)
        out.append((dict(board), "wb"[k & 1]))
        for i, pc in enumerate(ORDER):
            board[free[i]] = pc
            out.append((dict(board), "wb"[(i + k) & 1]))
    return out


def hand_made() -> np.ndarray:
    return np.stack([F.pos_from_fen(fen_of(b, stm)) for b, stm in ladder_boards()])


def hand_made_variant(variant: int) -> np.ndarray:
    boards = [(b, stm) for b, stm in ladder_boards() if len(b) <= 28]
    pos = [F.vpos_from_fen(variant, fen_of(b, stm)) for b, stm in boards]
    if variant == CZH:  # pockets of 1..4 pieces beside every board: lists of up to 32, buckets by the board alone
        pockets = ["P", "pQ", "NnB", "RrPp"]
        pos += [F.vpos_from_fen(variant, fen_of(b, stm, pockets[i & 3])) for i, (b, stm) in enumerate(boards)]
    return np.stack(pos)


def device_eval(ev, pos, variant=False):
    import torch
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(np.ascontiguousarray(pos)).to(dev)
    d_ps = torch.zeros(len(pos), dtype=torch.int32, device=dev)
    d_po = torch.zeros(len(pos), dtype=torch.int32, device=dev)
    call = ev.eval_vpositions_device if variant else ev.eval_positions_device
    call(d_pos.data_ptr(), len(pos), d_ps.data_ptr(), d_po.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ev.check()
    return d_ps.cpu().numpy(), d_po.cpu().numpy()


@pytest.fixture(scope="module")
def inputs():
    hand = hand_made()
    counts = sorted({int(np.count_nonzero(np.concatenate([p[:32] & 15, p[:32] >> 4]))) for p in hand})
    assert counts == list(range(2, 33))
    return {"hand": hand,
            "random": F.random_playouts(91, 4000, 0, 160, threads=8),
            "both": np.concatenate([hand, F.random_playouts(92, 3000, 0, 160, threads=8)])}


@pytest.fixture(scope="module")
def chess_nets():
    made = {}
    for hd in (128, 1024):
        data = F.synthesize_net(3, hd, 0)
        ev = F.Evaluator(F.Net.from_bytes(data), 0)
        ev.set_ft_impl(N.FT_SLICED)
        made[hd] = (ev, OracleNet(data), {})
    yield made
    for ev, _, _ in made.values():
        ev.close()


MASKS = {128: {"swar": 0b11, "packed": 0, "mixed": 0b10}, 1024: {"swar": 0xFFFF, "packed": 0, "mixed": 0xA5A4}}


@pytest.mark.parametrize("name", ["hand", "random", "both"])
@pytest.mark.parametrize("mode", ["swar", "packed", "mixed"])
@pytest.mark.parametrize("hd", [128, 1024])
def test_chess_bit_exact(chess_nets, inputs, hd, mode, name):
    ev, on, answers = chess_nets[hd]
    pos = inputs[name]
    if name not in answers:
        ops, opo, rc = on.eval_packed(pos, threads=8)
        assert rc == 0
        answers[name] = (ops, opo)
    ops, opo = answers[name]
    if name == "both":  # every bucket occurs (playouts rarely end below 5 pieces: bucket 0 is the ladder's)
        cnt = np.array([np.count_nonzero(np.concatenate([p[:32] & 15, p[:32] >> 4])) for p in pos])
        assert set(((cnt - 1) // 4).tolist()) == set(range(8))
    mask = MASKS[hd][mode]
    try:
        ev.set_swar_slices(mask)
        assert ev.swar_slices()[1] == mask
        ps, po = device_eval(ev, pos)
    finally:
        ev.set_swar(True)
    assert np.array_equal(ps, ops), f"psqt differs at {np.nonzero(ps != ops)[0][:8].tolist()}"
    assert np.array_equal(po, opo), f"positional differs at {np.nonzero(po != opo)[0][:8].tolist()}"


@pytest.mark.parametrize("mode", ["swar", "packed", "mixed"])
@pytest.mark.parametrize("variant", [CZH, ATOMIC], ids=["crazyhouse", "atomic"])
def test_variants_bit_exact(variant, mode):
    data = F.synthesize_variant_net(3, 256, variant, 0)
    ev, on = F.Evaluator(F.Net.from_bytes_variant(data, variant), 0), VariantOracleNet(data, variant)
    try:
        pos = np.concatenate([hand_made_variant(variant), F.random_vpositions(93, variant, 3000, 160)])
        if variant == CZH:  # pockets are filled in the playouts too
            assert len(pos) > 3000
        ops, opo, rc = on.eval_packed(pos, threads=8)
        assert rc == 0
        mask = {"swar": 0b1111, "packed": 0, "mixed": 0b0110}[mode]
        ev.set_swar_slices(mask)
        assert ev.swar_slices()[1] == mask
        ps, po = device_eval(ev, pos, variant=True)
        assert np.array_equal(ps, ops), f"psqt differs at {np.nonzero(ps != ops)[0][:8].tolist()}"
        assert np.array_equal(po, opo), f"positional differs at {np.nonzero(po != opo)[0][:8].tolist()}"
    finally:
        ev.close()

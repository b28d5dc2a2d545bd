"""Host-side API of the MI355X NNUE evaluator over the C ABI.

Mirrors what the reference does on its static-evaluation path:

* ``Net.load(path)`` — ``setoption name EvalFile value <path>``
  ([ref] src/stockfish.rs:209-211; net file from src/assets.rs:128-133).
* ``Evaluator(net, device)`` — one engine per worker becomes one context per
  GPU ([ref] src/stockfish.rs:23-38 ``channel``; src/main.rs:158-170).
* ``Evaluator.eval_positions`` / ``eval_groups`` — batched replacement for one
  ``position fen ... moves ...`` round trip per position
  ([ref] src/stockfish.rs:274-283).
* ``game_positions`` — the per-ply expansion of an analysis batch
  ([ref] src/queue.rs:543-600, ``IncomingBatch::from_acquired``).

Errors raise :class:`FnnueError`; the caller treats any of them as
``PositionFailed`` for the whole batch ([ref] src/queue.rs:207-213).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._native import FnnueError  # noqa: F401  (re-export)


class Net:
    """A parsed and validated .nnue network (immutable, shareable)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    @classmethod
    def load(cls, path: str) -> "Net":
        h = C.c_void_p()
        N.check(N.lib.fnnue_net_load(path.encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def load_variant(cls, path: str, variant: int) -> "Net":
        """A Fairy-Stockfish variant net (VARIANT_CRAZYHOUSE / VARIANT_ATOMIC /
        VARIANT_KINGOFTHEHILL / VARIANT_RACINGKINGS / VARIANT_THREECHECK; the last four share one
        file format)."""
        h = C.c_void_p()
        N.check(N.lib.fnnue_net_load_variant(path.encode(), variant, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_bytes_variant(cls, data: bytes, variant: int) -> "Net":
        h = C.c_void_p()
        buf = C.create_string_buffer(data, len(data))
        N.check(N.lib.fnnue_net_load_variant_mem(buf, len(data), variant, C.byref(h)))
        return cls(h.value)

    @property
    def variant(self) -> int:
        v = C.c_int()
        N.check(N.lib.fnnue_net_variant(self._h, C.byref(v)))
        return v.value

    @classmethod
    def from_bytes(cls, data: bytes) -> "Net":
        h = C.c_void_p()
        buf = C.create_string_buffer(data, len(data))
        N.check(N.lib.fnnue_net_load_mem(buf, len(data), C.byref(h)))
        return cls(h.value)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> tuple[int, int, str]:
        hd, fh, desc = C.c_uint32(), C.c_uint32(), C.c_char_p()
        N.check(N.lib.fnnue_net_info(self._h, C.byref(hd), C.byref(fh), C.byref(desc)))
        return hd.value, fh.value, desc.value.decode(errors="replace")

    def sha256(self) -> str:
        """SHA-256 of the file bytes, lowercase hex (net identity)."""
        d = (C.c_uint8 * 32)()
        N.check(N.lib.fnnue_net_sha256(self._h, d))
        return bytes(d).hex()

    def accumulator_bound(self) -> int:
        """Largest possible |sum| of an even accumulator column (< 2^15: SWAR rows exact)."""
        b = C.c_int32()
        N.check(N.lib.fnnue_net_accumulator_bound(self._h, C.byref(b)))
        return b.value

    def slice_bounds(self) -> np.ndarray:
        """The accumulator bound of every 64-column slice (int32, hd / 64 values; their
        maximum is accumulator_bound()).  A slice below 2^15 runs SWAR rows."""
        out = np.zeros(64, dtype=np.int32)
        n = C.c_size_t()
        N.check(N.lib.fnnue_net_slice_bounds(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out), C.byref(n)))
        return out[: n.value].copy()

    def image(self) -> np.ndarray:
        size = C.c_size_t()
        N.check(N.lib.fnnue_net_image_size(self._h, C.byref(size)))
        buf = np.zeros(size.value, dtype=np.uint8)
        N.check(N.lib.fnnue_net_image_pack(self._h, N.ptr(buf), size.value))
        return buf

    def __del__(self):
        # at interpreter shutdown the module globals may already be gone
        lib = getattr(N, "lib", None) if N is not None else None
        if lib is not None and getattr(self, "_h", None) and self._h.value:
            lib.fnnue_net_free(self._h)
            self._h = C.c_void_p()


def synthesize_net(seed: int, hd: int = 1024, flags: int = 0) -> bytes:
    """Deterministic synthetic net in the exact .nnue format."""
    buf, size = C.c_void_p(), C.c_size_t()
    N.check(N.lib.fnnue_net_synthesize(seed, hd, flags, C.byref(buf), C.byref(size)))
    try:
        return C.string_at(buf.value, size.value)
    finally:
        N.lib.fnnue_buffer_free(buf)


def synthesize_variant_net(seed: int, hd: int, variant: int, flags: int = 0) -> bytes:
    """Deterministic synthetic Fairy-Stockfish variant net in the .nnue format."""
    buf, size = C.c_void_p(), C.c_size_t()
    N.check(N.lib.fnnue_net_synthesize_variant(seed, hd, variant, flags, C.byref(buf), C.byref(size)))
    try:
        return C.string_at(buf.value, size.value)
    finally:
        N.lib.fnnue_buffer_free(buf)


def vpos_from_fen(variant: int, fen: str) -> np.ndarray:
    out = N.vpositions_array(1)
    N.check(N.lib.fnnue_vpos_from_fen(variant, fen.encode(), N.ptr(out)))
    return out[0]


def random_vpositions(seed: int, variant: int, count: int, max_plies: int = 120, mode: int = N.PLAYOUT_FINAL):
    """Seeded pseudo-legal random walks of a variant (test inputs).  FINAL ->
    positions; PLIES -> (positions, CHAIN group offsets)."""
    cap = count if mode == N.PLAYOUT_FINAL else count * (max_plies + 1)
    out = N.vpositions_array(cap)
    off = np.zeros(count + 1, dtype=np.uint32)
    n, g = C.c_size_t(), C.c_size_t()
    N.check(N.lib.fnnue_random_vpositions(seed, variant, count, max_plies, mode, N.ptr(out), cap, N.ptr(off), len(off),
                                          C.byref(n), C.byref(g)))
    if mode == N.PLAYOUT_FINAL:
        return out[: n.value]
    return out[: n.value], off[: g.value + 1]


def game_vpositions(variant: int, fen: str, moves: str | list[str]) -> np.ndarray:
    """Root + the position after every move of a variant game (host replay)."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    n = C.c_size_t()
    cap = moves.count(" ") + 2 if moves.strip() else 1
    out = N.vpositions_array(cap)
    N.check(N.lib.fnnue_game_vpositions(variant, fen.encode(), moves.encode(), N.ptr(out), cap, C.byref(n)))
    return out[: n.value]


def game_vchildren(variant: int, fen: str, moves: str | list[str]) -> tuple[np.ndarray, np.ndarray]:
    """Every ply of a variant game plus its legal children (drops included), STAR groups."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    nply = (moves.count(" ") + 2) if moves.strip() else 1
    n, g = C.c_size_t(), C.c_size_t()
    off = np.zeros(nply + 1, dtype=np.uint32)
    rc = N.lib.fnnue_game_vchildren(variant, fen.encode(), moves.encode(), None, 0, N.ptr(off), len(off),
                                    C.byref(n), C.byref(g))
    if rc != -10:
        N.check(rc)
    out = N.vpositions_array(n.value)
    N.check(N.lib.fnnue_game_vchildren(variant, fen.encode(), moves.encode(), N.ptr(out), len(out), N.ptr(off),
                                       len(off), C.byref(n), C.byref(g)))
    return out[: n.value], off[: g.value + 1]


END_NO_MOVES, END_CHECK, END_EXTINCT = 1, 2, 4
END_VARIANT = 8  # the game is decided by the variant's own rule (kingofthehill, racingkings, threecheck)
END_WON = 0x40   # on a child of build_vchildren: its side to move has already won (the mover lost by playing it)


END_DRAW = N.END_DRAW  # on a searched record: drawn by repetition or the fifty-move rule (ABI 3.12)
# fnnue_ply_history: a ply's halfmove clock and the number of earlier plies of its game with its identity
PLY_HISTORY_DTYPE = np.dtype([("clock", "<u2"), ("seen", "u1"), ("reserved", "u1")])


def _game_history(fn, head, games) -> tuple[np.ndarray, np.ndarray]:
    text, fen_off, mv_off = pack_games(games)
    cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
    out = np.zeros(max(cap, 1), dtype=PLY_HISTORY_DTYPE)
    off = np.zeros(len(games) + 1, dtype=np.uint32)
    n, g = C.c_size_t(), C.c_size_t()
    N.check(fn(*head, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), N.ptr(out), cap, N.ptr(off),
               len(off), C.byref(n), C.byref(g)))
    return out[: n.value], off[: g.value + 1]


def game_history(games) -> tuple[np.ndarray, np.ndarray]:
    """fnnue_game_history (host replay): every ply's clock and `seen` of every (fen, moves) game
    -> (PLY_HISTORY_DTYPE records, CHAIN offsets per game)."""
    return _game_history(N.lib.fnnue_game_history, (), games)


def game_vhistory(variant: int, games) -> tuple[np.ndarray, np.ndarray]:
    """fnnue_game_vhistory (host variant replay): game_history() under the variant's rule (ABI 3.16: crazyhouse
    has no clock and counts pockets and promoted marks, threecheck counts its check counters)."""
    return _game_history(N.lib.fnnue_game_vhistory, (variant,), games)


def game_end(fen: str, moves: str | list[str] = "", variant: int = 0) -> int:
    """FNNUE_END_* flags of the position after `moves` (host replay): no legal
    move, side to move in check, its king exploded (atomic)."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    flags = C.c_int()
    N.check(N.lib.fnnue_game_end(variant, fen.encode(), moves.encode(), C.byref(flags)))
    return flags.value


def vperft(variant: int, fen: str, depth: int) -> int:
    nodes = C.c_uint64()
    N.check(N.lib.fnnue_vperft(variant, fen.encode(), depth, C.byref(nodes)))
    return nodes.value


def random_vgame(seed: int, variant: int, fen: str, plies: int) -> str:
    """Up to `plies` random legal moves of a variant game as UCI (drops "N@f3")."""
    n = C.c_size_t()
    buf = C.create_string_buffer(8 * plies + 16)
    N.check(N.lib.fnnue_random_vgame(seed, variant, fen.encode(), plies, buf, len(buf), C.byref(n)))
    return buf.value.decode()


def random_vgames(seed: int, variant: int, count: int, max_plies: int = 160, threads: int = 8):
    """Every ply of seeded random legal variant games, CHAIN groups -> (positions, offsets)."""
    cap = count * (max_plies + 1)
    out = N.vpositions_array(cap)
    off = np.zeros(count + 1, dtype=np.uint32)
    n, g = C.c_size_t(), C.c_size_t()
    N.check(N.lib.fnnue_random_vgames(seed, variant, count, max_plies, threads, N.ptr(out), cap, N.ptr(off), len(off),
                                      C.byref(n), C.byref(g)))
    return out[: n.value], off[: g.value + 1]


class Best(C.Structure):
    """fnnue_best: the result of a one-ply search over one position's children."""
    _fields_ = [("psqt", C.c_int32), ("positional", C.c_int32), ("value", C.c_int32), ("nodes", C.c_uint32),
                ("best", C.c_uint32), ("move", C.c_uint16), ("kind", C.c_uint8), ("end", C.c_uint8)]


BEST_DTYPE = np.dtype([("psqt", "<i4"), ("positional", "<i4"), ("value", "<i4"), ("nodes", "<u4"), ("best", "<u4"),
                       ("move", "<u2"), ("kind", "u1"), ("end", "u1")])
BEST_NONE, BEST_CP, BEST_MATE, BEST_LOST = N.BEST_NONE, N.BEST_CP, N.BEST_MATE, N.BEST_LOST
# fnnue_best2: the result of a two-ply search over one position (kind BEST_MATED: every move allows a mate in one)
BEST2_DTYPE = np.dtype([("psqt", "<i4"), ("positional", "<i4"), ("value", "<i4"), ("nodes", "<u4"), ("best", "<u4"),
                        ("reply_index", "<u4"), ("move", "<u2"), ("reply", "<u2"), ("kind", "u1"), ("end", "u1"),
                        ("pv_len", "u1"), ("reserved", "u1")])
BEST_MATED = N.BEST_MATED


class Line(C.Structure):
    """fnnue_line: one of a group's k best children (MultiPV at depth 1); kind BEST_NONE = an unused slot."""
    _fields_ = [("psqt", C.c_int32), ("positional", C.c_int32), ("value", C.c_int32), ("child", C.c_uint32),
                ("move", C.c_uint16), ("kind", C.c_uint8), ("reserved", C.c_uint8)]


LINE_DTYPE = np.dtype([("psqt", "<i4"), ("positional", "<i4"), ("value", "<i4"), ("child", "<u4"), ("move", "<u2"),
                       ("kind", "u1"), ("reserved", "u1")])
MAX_CHILDREN = N.MAX_CHILDREN
# fnnue_quiet (ABI 3.13): Q_d of a position, the terms of its capture line's end, the line's first move
QUIET_DTYPE = np.dtype([("psqt", "<i4"), ("positional", "<i4"), ("value", "<i4"), ("nodes", "<u4"), ("move", "<u2"),
                        ("len", "u1"), ("reserved", "u1")])
QUIESCE_MAX = 4
VALUE_MATE = 32000     # FNNUE_VALUE_MATE (ABI 3.14): the value of a mated position under quiescence checks
QUIET_DECIDED = 1      # FNNUE_QUIET_DECIDED in QUIET_DTYPE's "reserved" byte
# fnnue_line2: one of a ply's k best lines at two plies (move, reply); kind BEST_NONE = an unused slot
LINE2_DTYPE = np.dtype([("psqt", "<i4"), ("positional", "<i4"), ("value", "<i4"), ("child", "<u4"),
                        ("reply_index", "<u4"), ("move", "<u2"), ("reply", "<u2"), ("kind", "u1"), ("pv_len", "u1"),
                        ("reserved", "<u2")])


def move_uci(code: int) -> str:
    """A fnnue_move code as UCI text ("" for 0); FnnueError FNNUE_E_ARG for a code that is no move."""
    buf = C.create_string_buffer(8)
    N.check(N.lib.fnnue_move_uci(int(code), buf))
    return buf.value.decode()


def vmove_uci(code: int) -> str:
    """A variant move code as UCI text (fnnue_vmove_uci): as move_uci, and a drop (from == to, the piece
    type in the promo field) as "N@f3"; FnnueError FNNUE_E_ARG for a code that is neither."""
    buf = C.create_string_buffer(8)
    N.check(N.lib.fnnue_vmove_uci(int(code), buf))
    return buf.value.decode()


def device_count() -> int:
    n = C.c_int()
    N.check(N.lib.fnnue_device_count(C.byref(n)))
    return n.value


class Evaluator:
    """A net resident on one GPU (one per process/GPU)."""

    def __init__(self, net: Net | None, device: int = 0, *, image_ptr: int | None = None,
                 image_bytes: int = 0, hd: int = 0):
        h = C.c_void_p()
        if net is not None:
            N.check(N.lib.fnnue_ctx_create(net.handle, device, C.byref(h)))
        else:
            N.check(N.lib.fnnue_ctx_create_from_image(device, hd, C.c_void_p(image_ptr), image_bytes, C.byref(h)))
        self._h = h
        self.device = device

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def device_image(self) -> tuple[int, int]:
        p, s = C.c_void_p(), C.c_size_t()
        N.check(N.lib.fnnue_ctx_image(self._h, C.byref(p), C.byref(s)))
        return p.value, s.value

    def eval_positions(self, pos: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        pos = np.ascontiguousarray(pos, dtype=np.uint8).reshape(-1, N.POS_BYTES)
        n = pos.shape[0]
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_eval_positions(self._h, N.ptr(pos), n, N.ptr(psqt), N.ptr(positional)))
        return psqt, positional

    def eval_groups(self, pos: np.ndarray, off: np.ndarray, mode: int = N.GROUP_CHAIN):
        pos = np.ascontiguousarray(pos, dtype=np.uint8).reshape(-1, N.POS_BYTES)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        if len(off) < 1:
            raise ValueError("off needs at least one entry (off[0] = 0)")
        n = pos.shape[0]
        if int(off[-1]) != n:
            raise ValueError(f"off[-1] = {int(off[-1])} but {n} positions were given")
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_eval_groups(self._h, N.ptr(pos), n, N.ptr(off), len(off) - 1, mode,
                                        N.ptr(psqt), N.ptr(positional)))
        return psqt, positional

    def eval_vpositions(self, vpos: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """Fairy-Stockfish variant positions (fnnue_vpos, 48 B) on a variant-net context."""
        vpos = np.ascontiguousarray(vpos, dtype=np.uint8).reshape(-1, N.VPOS_BYTES)
        n = vpos.shape[0]
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_eval_vpositions(self._h, N.ptr(vpos), n, N.ptr(psqt), N.ptr(positional)))
        return psqt, positional

    def eval_vgroups(self, vpos: np.ndarray, off: np.ndarray, mode: int = N.GROUP_CHAIN):
        """Variant positions in CHAIN / STAR groups, accumulators carried along (incremental)."""
        vpos = np.ascontiguousarray(vpos, dtype=np.uint8).reshape(-1, N.VPOS_BYTES)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        if len(off) < 1 or int(off[-1]) != vpos.shape[0]:
            raise ValueError("off must have >= 1 entry and end at the number of positions")
        n = vpos.shape[0]
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_eval_vgroups(self._h, N.ptr(vpos), n, N.ptr(off), len(off) - 1, mode, N.ptr(psqt),
                                         N.ptr(positional)))
        return psqt, positional

    def eval_vgroups_device(self, d_pos: int, d_off: int, ngroups: int, npos: int, mode: int, d_psqt: int,
                            d_positional: int, stream: int | None):
        N.check(N.lib.fnnue_eval_vgroups_device(self._h, C.c_void_p(d_pos), C.c_void_p(d_off), ngroups, npos, mode,
                                                C.c_void_p(d_psqt), C.c_void_p(d_positional), C.c_void_p(stream)))

    def eval_vpositions_device(self, d_pos: int, n: int, d_psqt: int, d_positional: int, stream: int | None):
        N.check(N.lib.fnnue_eval_vpositions_device(self._h, C.c_void_p(d_pos), n, C.c_void_p(d_psqt),
                                                   C.c_void_p(d_positional), C.c_void_p(stream)))

    # Device-pointer entry points (inputs resident in HBM; asynchronous).
    def eval_positions_device(self, d_pos: int, n: int, d_psqt: int, d_positional: int, stream: int | None):
        N.check(N.lib.fnnue_eval_positions_device(self._h, C.c_void_p(d_pos), n, C.c_void_p(d_psqt),
                                                  C.c_void_p(d_positional), C.c_void_p(stream)))

    def eval_groups_device(self, d_pos: int, d_off: int, ngroups: int, npos: int, mode: int, d_psqt: int,
                           d_positional: int, stream: int | None):
        N.check(N.lib.fnnue_eval_groups_device(self._h, C.c_void_p(d_pos), C.c_void_p(d_off), ngroups, npos, mode,
                                               C.c_void_p(d_psqt), C.c_void_p(d_positional), C.c_void_p(stream)))

    def eval_groups_dual_device(self, small: "Evaluator", d_pos: int, d_off: int, ngroups: int, npos: int, mode: int,
                                d_psqt: int, d_positional: int, d_psqt_small: int, d_positional_small: int,
                                stream: int | None):
        """This (big) net and `small` over the same groups, one plan (fnnue_eval_groups_dual_device)."""
        N.check(N.lib.fnnue_eval_groups_dual_device(self._h, small._h, C.c_void_p(d_pos), C.c_void_p(d_off), ngroups,
                                                    npos, mode, C.c_void_p(d_psqt), C.c_void_p(d_positional),
                                                    C.c_void_p(d_psqt_small), C.c_void_p(d_positional_small),
                                                    C.c_void_p(stream)))

    def eval_groups_dual(self, small: "Evaluator", pos: np.ndarray, off: np.ndarray, mode: int = N.GROUP_CHAIN):
        """Host-buffer convenience over eval_groups_dual_device (torch for the device buffers)."""
        import torch
        dev = torch.device("cuda", self.device)
        pos = np.ascontiguousarray(pos, dtype=np.uint8).reshape(-1, N.POS_BYTES)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(pos)
        d_pos = torch.from_numpy(pos).to(dev)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        out = torch.zeros((4, max(n, 1)), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.eval_groups_dual_device(small, d_pos.data_ptr(), d_off.data_ptr(), len(off) - 1, n, mode,
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None)
        self.check()
        small.check()
        o = out[:, :n].cpu().numpy()
        return o[0], o[1], o[2], o[3]

    def check(self) -> None:
        N.check(N.lib.fnnue_ctx_check(self._h))

    # Device-side batch builder (fnnue_build_batch): games = [(fen, "uci uci ..."), ...].
    def build_batch(self, games, mode: int = N.PLAYOUT_PLIES) -> tuple[np.ndarray, np.ndarray]:
        text, fen_off, mv_off = pack_games(games)
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_build_batch(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), mode,
                                     None, 0, None, 0, C.byref(n), C.byref(g))
        if rc != -10:  # FNNUE_E_CAPACITY reports the sizes; anything else is final
            N.check(rc)
            return N.positions_array(0), np.zeros(1, dtype=np.uint32)
        out = N.positions_array(n.value)
        off = np.zeros(g.value + 1, dtype=np.uint32)
        N.check(N.lib.fnnue_build_batch(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), mode,
                                        N.ptr(out), len(out), N.ptr(off), len(off), C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1]

    # Variant games on the device (fnnue_build_vbatch): games = [(fen, "uci ..."), ...].
    def build_vbatch(self, variant: int, games, mode: int = N.PLAYOUT_PLIES) -> tuple[np.ndarray, np.ndarray]:
        text, fen_off, mv_off = pack_games(games)
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_build_vbatch(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                      mode, None, 0, None, 0, C.byref(n), C.byref(g))
        if rc != -10:
            N.check(rc)
            return N.vpositions_array(0), np.zeros(1, dtype=np.uint32)
        out = N.vpositions_array(n.value)
        off = np.zeros(g.value + 1, dtype=np.uint32)
        N.check(N.lib.fnnue_build_vbatch(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off),
                                         len(games), mode, N.ptr(out), len(out), N.ptr(off), len(off), C.byref(n),
                                         C.byref(g)))
        return out[: n.value], off[: g.value + 1]

    # The one-ply search (ABI 3.4): games = [(fen, "uci uci ..."), ...].
    def build_children(self, games):
        """fnnue_build_children: (records, STAR offsets, move codes, end flags) of every ply and its children."""
        text, fen_off, mv_off = pack_games(games)
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_build_children(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), None, 0,
                                        None, 0, None, None, C.byref(n), C.byref(g))
        if rc != -10:
            N.check(rc)
            return N.positions_array(0), np.zeros(1, dtype=np.uint32), np.zeros(0, np.uint16), np.zeros(0, np.uint8)
        out = N.positions_array(n.value)
        off = np.zeros(g.value + 1, dtype=np.uint32)
        moves = np.zeros(n.value, dtype=np.uint16)
        end = np.zeros(n.value, dtype=np.uint8)
        N.check(N.lib.fnnue_build_children(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                           N.ptr(out), len(out), N.ptr(off), len(off), N.ptr(moves), N.ptr(end),
                                           C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1], moves[: n.value], end[: n.value]

    def build_children_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, d_out: int, cap: int,
                              d_off: int, off_cap: int, d_moves: int, d_end: int, stream: int | None):
        """fnnue_build_children_device -> (rc, records, groups); rc is FNNUE_E_CAPACITY (-10) on a sizing call."""
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_build_children_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                               C.c_void_p(d_moves_off), ngames, C.c_void_p(d_out), cap,
                                               C.c_void_p(d_off), off_cap, C.c_void_p(d_moves), C.c_void_p(d_end),
                                               C.byref(n), C.byref(g), C.c_void_p(stream))
        if rc != -10:
            N.check(rc)
        return rc, n.value, g.value

    def best_children(self, psqt, positional, end, moves, off) -> np.ndarray:
        """fnnue_best_children: one BEST_DTYPE record per STAR group (moves may be None)."""
        psqt = np.ascontiguousarray(psqt, dtype=np.int32)
        positional = np.ascontiguousarray(positional, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        if moves is not None:
            moves = np.ascontiguousarray(moves, dtype=np.uint16)
        out = np.zeros(len(off) - 1, dtype=BEST_DTYPE)
        N.check(N.lib.fnnue_best_children(self._h, N.ptr(psqt), N.ptr(positional), N.ptr(end), N.ptr(moves),
                                          N.ptr(off), len(off) - 1, len(psqt), N.ptr(out)))
        return out

    def best_children_device(self, d_psqt: int, d_positional: int, d_end: int, d_moves: int | None, d_off: int,
                             ngroups: int, npos: int, d_out: int, stream: int | None):
        N.check(N.lib.fnnue_best_children_device(self._h, C.c_void_p(d_psqt), C.c_void_p(d_positional),
                                                 C.c_void_p(d_end), C.c_void_p(d_moves), C.c_void_p(d_off), ngroups,
                                                 npos, C.c_void_p(d_out), C.c_void_p(stream)))

    def search1(self, games) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_search1: a one-ply search per ply -> (BEST_DTYPE records, CHAIN offsets per game)."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=BEST_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_search1(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), N.ptr(out),
                                    cap, N.ptr(off), len(off), C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1]

    def search1_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, d_out: int, cap: int,
                       d_off: int, off_cap: int, stream: int | None) -> tuple[int, int]:
        """fnnue_search1_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_search1_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off), C.c_void_p(d_moves_off),
                                           ngames, C.c_void_p(d_out), cap, C.c_void_p(d_off), off_cap, C.byref(n),
                                           C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    # repetition and fifty-move draws (ABI 3.12)
    def set_search_draws(self, on: bool) -> None:
        """fnnue_set_search_draws: search1 / search1_lines / search2 / search2_lines mark the searched
        positions drawn by repetition or the fifty-move rule (END_DRAW: worth 0, the pv ends there)."""
        N.check(N.lib.fnnue_set_search_draws(self._h, 1 if on else 0))

    def search_draws(self) -> bool:
        on = C.c_int()
        N.check(N.lib.fnnue_get_search_draws(self._h, C.byref(on)))
        return bool(on.value)

    def game_history(self, games) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_ctx_game_history: game_history() computed on the device from the replay's boards."""
        return _game_history(N.lib.fnnue_ctx_game_history, (self._h,), games)

    def game_history_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, d_out: int, cap: int,
                            d_off: int, off_cap: int, stream: int | None) -> tuple[int, int]:
        """fnnue_game_history_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_game_history_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                                C.c_void_p(d_moves_off), ngames, C.c_void_p(d_out), cap,
                                                C.c_void_p(d_off), off_cap, C.byref(n), C.byref(g),
                                                C.c_void_p(stream)))
        return n.value, g.value

    # repetition and fifty-move draws in the variant searches (ABI 3.16)
    def set_search_vdraws(self, on: bool) -> None:
        """fnnue_set_search_vdraws: vsearch1 / vsearch1_lines / vsearch2 / vsearch2_lines mark the searched
        positions drawn under their variant's rule (END_DRAW); a chess net's context ignores it."""
        N.check(N.lib.fnnue_set_search_vdraws(self._h, 1 if on else 0))

    def search_vdraws(self) -> bool:
        on = C.c_int()
        N.check(N.lib.fnnue_get_search_vdraws(self._h, C.byref(on)))
        return bool(on.value)

    def game_vhistory(self, variant: int, games) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_ctx_game_vhistory: game_vhistory() computed on the device from the variant replay's boards
        (any net's context serves)."""
        return _game_history(N.lib.fnnue_ctx_game_vhistory, (self._h, variant), games)

    # capture quiescence below the search's leaves (ABI 3.13)
    def set_search_quiesce(self, depth: int) -> None:
        """fnnue_set_search_quiesce: the leaves of search1 / search1_lines / search2 / search2_children /
        search2_lines take the terms of their capture line's end, `depth` captures deep at most (0: off)."""
        N.check(N.lib.fnnue_set_search_quiesce(self._h, depth))

    def search_quiesce(self) -> int:
        d = C.c_int()
        N.check(N.lib.fnnue_get_search_quiesce(self._h, C.byref(d)))
        return d.value

    def set_search_quiesce_checks(self, on: bool) -> None:
        """fnnue_set_search_quiesce_checks: the quiescence of the searches and of quiesce() follows Q' (ABI
        3.14): a node in check lists its evasions and may not stand pat, mates are values near VALUE_MATE."""
        N.check(N.lib.fnnue_set_search_quiesce_checks(self._h, 1 if on else 0))

    def search_quiesce_checks(self) -> bool:
        on = C.c_int()
        N.check(N.lib.fnnue_get_search_quiesce_checks(self._h, C.byref(on)))
        return bool(on.value)

    def quiesce_slices(self) -> int:
        """fnnue_quiesce_slices: the slices of leaves the context's quiescence has worked through so far."""
        n = C.c_uint64()
        N.check(N.lib.fnnue_quiesce_slices(self._h, C.byref(n)))
        return n.value

    def quiesce(self, games, depth: int) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_quiesce: Q_depth of every ply -> (QUIET_DTYPE records, CHAIN offsets per game)."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=QUIET_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_quiesce(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), depth,
                                    N.ptr(out), cap, N.ptr(off), len(off), C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1]

    def quiesce_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, depth: int, d_out: int,
                       cap: int, d_off: int, off_cap: int, stream: int | None) -> tuple[int, int]:
        """fnnue_quiesce_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_quiesce_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off), C.c_void_p(d_moves_off),
                                           ngames, depth, C.c_void_p(d_out), cap, C.c_void_p(d_off), off_cap,
                                           C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    # capture quiescence for the variant searches (ABI 3.15)
    def set_search_vquiesce(self, depth: int, checks: bool = False) -> None:
        """fnnue_set_search_vquiesce: the leaves of vsearch1 / vsearch1_lines / vsearch2 / vsearch2_children /
        vsearch2_lines take the terms of their capture line's end under the variant's rule, `depth` captures
        deep at most (0: off); `checks`: nodes in check list their evasions (drops included) and may be mated."""
        N.check(N.lib.fnnue_set_search_vquiesce(self._h, depth, 1 if checks else 0))

    def search_vquiesce(self) -> tuple[int, bool]:
        d, on = C.c_int(), C.c_int()
        N.check(N.lib.fnnue_get_search_vquiesce(self._h, C.byref(d), C.byref(on)))
        return d.value, bool(on.value)

    def vquiesce(self, variant: int, games, depth: int, checks: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_vquiesce: the variant's Q_depth of every ply -> (QUIET_DTYPE records, CHAIN offsets per game)."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=QUIET_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vquiesce(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                     depth, 1 if checks else 0, N.ptr(out), cap, N.ptr(off), len(off), C.byref(n),
                                     C.byref(g)))
        return out[: n.value], off[: g.value + 1]

    def vquiesce_device(self, variant: int, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, depth: int,
                        checks: bool, d_out: int, cap: int, d_off: int, off_cap: int,
                        stream: int | None) -> tuple[int, int]:
        """fnnue_vquiesce_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vquiesce_device(self._h, variant, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                            C.c_void_p(d_moves_off), ngames, depth, 1 if checks else 0,
                                            C.c_void_p(d_out), cap, C.c_void_p(d_off), off_cap, C.byref(n), C.byref(g),
                                            C.c_void_p(stream)))
        return n.value, g.value

    # the two-ply search (ABI 3.7)
    def best_replies(self, end, moves, off, child_best) -> np.ndarray:
        """fnnue_best_replies: the second reduction, one BEST2_DTYPE record per STAR group from the
        level-1 end flags and moves (moves may be None) and the children's BEST_DTYPE records
        (dense, in record order)."""
        end = np.ascontiguousarray(end, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        child_best = np.ascontiguousarray(child_best, dtype=BEST_DTYPE)
        if moves is not None:
            moves = np.ascontiguousarray(moves, dtype=np.uint16)
        out = np.zeros(len(off) - 1, dtype=BEST2_DTYPE)
        N.check(N.lib.fnnue_best_replies(self._h, N.ptr(end), N.ptr(moves), N.ptr(off), len(off) - 1, len(end),
                                         N.ptr(child_best), N.ptr(out)))
        return out

    def best_replies_device(self, d_end: int, d_moves: int | None, d_off: int, ngroups: int, npos: int,
                            d_child_best: int, d_out: int, stream: int | None):
        N.check(N.lib.fnnue_best_replies_device(self._h, C.c_void_p(d_end), C.c_void_p(d_moves), C.c_void_p(d_off),
                                                ngroups, npos, C.c_void_p(d_child_best), C.c_void_p(d_out),
                                                C.c_void_p(stream)))

    def search2(self, games, children: bool = False):
        """fnnue_search2: a two-ply search per ply -> (BEST2_DTYPE records, CHAIN offsets per game).
        With `children` (fnnue_search2_children) also the children's depth-1 records and their
        (ply, 1-based child index) pairs: -> (records, offsets, BEST_DTYPE records, (n, 2) uint32)."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=BEST2_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        if not children:
            N.check(N.lib.fnnue_search2(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                        N.ptr(out), cap, N.ptr(off), len(off), C.byref(n), C.byref(g)))
            return out[: n.value], off[: g.value + 1]
        kcap = cap * MAX_CHILDREN
        kb = np.zeros(max(kcap, 1), dtype=BEST_DTYPE)
        km = np.zeros((max(kcap, 1), 2), dtype=np.uint32)
        nk = C.c_size_t()
        N.check(N.lib.fnnue_search2_children(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                             N.ptr(out), cap, N.ptr(off), len(off), N.ptr(kb), N.ptr(km), kcap,
                                             C.byref(n), C.byref(g), C.byref(nk)))
        return out[: n.value], off[: g.value + 1], kb[: nk.value], km[: nk.value]

    def search2_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, d_out: int, cap: int,
                       d_off: int, off_cap: int, stream: int | None) -> tuple[int, int]:
        """fnnue_search2_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_search2_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off), C.c_void_p(d_moves_off),
                                           ngames, C.c_void_p(d_out), cap, C.c_void_p(d_off), off_cap, C.byref(n),
                                           C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    # MultiPV at depth 1 (ABI 3.5)
    def topk_children(self, psqt, positional, end, moves, off, k_or_line_off, lines_cap: int | None = None,
                      fill: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_topk_children: the k best children of every STAR group -> (LINE_DTYPE slots, line_off).
        `k_or_line_off`: one slot count for every group, or the ngroups + 1 slot offsets.  `lines_cap`
        (default: line_off[-1]) sizes the buffer; its bytes start as `fill`, so that a caller can
        see which slots were written."""
        psqt = np.ascontiguousarray(psqt, dtype=np.int32)
        positional = np.ascontiguousarray(positional, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        if moves is not None:
            moves = np.ascontiguousarray(moves, dtype=np.uint16)
        ng = len(off) - 1
        if np.ndim(k_or_line_off) == 0:
            line_off = (np.arange(ng + 1, dtype=np.uint64) * int(k_or_line_off)).astype(np.uint32)
        else:
            line_off = np.ascontiguousarray(k_or_line_off, dtype=np.uint32)
        cap = int(line_off[-1]) if lines_cap is None else int(lines_cap)
        lines = np.full(max(cap, 1) * N.LINE_BYTES, fill, dtype=np.uint8).view(LINE_DTYPE)
        N.check(N.lib.fnnue_topk_children(self._h, N.ptr(psqt), N.ptr(positional), N.ptr(end), N.ptr(moves),
                                          N.ptr(off), ng, len(psqt), N.ptr(line_off), N.ptr(lines), cap))
        return lines[:cap], line_off

    def topk_children_device(self, d_psqt: int, d_positional: int, d_end: int, d_moves: int | None, d_off: int,
                             ngroups: int, npos: int, d_line_off: int, d_lines: int, lines_cap: int,
                             stream: int | None):
        N.check(N.lib.fnnue_topk_children_device(self._h, C.c_void_p(d_psqt), C.c_void_p(d_positional),
                                                 C.c_void_p(d_end), C.c_void_p(d_moves), C.c_void_p(d_off), ngroups,
                                                 npos, C.c_void_p(d_line_off), C.c_void_p(d_lines), lines_cap,
                                                 C.c_void_p(stream)))

    def search1_lines(self, games, k: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """fnnue_search1_lines: search1 plus each ply's k best children ->
        (BEST_DTYPE records, CHAIN offsets per game, LINE_DTYPE slots of shape (plies, k))."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=BEST_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        lines = np.zeros(max(cap * max(int(k), 0), 1), dtype=LINE_DTYPE)
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_search1_lines(self._h, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), int(k),
                                          N.ptr(out), cap, N.ptr(off), len(off), N.ptr(lines), cap * int(k),
                                          C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1], lines[: n.value * int(k)].reshape(n.value, int(k))

    def search1_lines_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, k: int, d_out: int,
                             cap: int, d_off: int, off_cap: int, d_lines: int, lines_cap: int,
                             stream: int | None) -> tuple[int, int]:
        """fnnue_search1_lines_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when a buffer is too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_search1_lines_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                                 C.c_void_p(d_moves_off), ngames, int(k), C.c_void_p(d_out), cap,
                                                 C.c_void_p(d_off), off_cap, C.c_void_p(d_lines), lines_cap,
                                                 C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    # The one-ply search of the Fairy-Stockfish variants (ABI 3.6): a variant net's context.
    def build_vchildren(self, variant: int, games):
        """fnnue_build_vchildren: (records, STAR offsets, variant move codes, end flags) of every ply and its
        children; a child's flags carry END_WON when its side to move has already won."""
        text, fen_off, mv_off = pack_games(games)
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_build_vchildren(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                         None, 0, None, 0, None, None, C.byref(n), C.byref(g))
        if rc != -10:
            N.check(rc)
            return N.vpositions_array(0), np.zeros(1, dtype=np.uint32), np.zeros(0, np.uint16), np.zeros(0, np.uint8)
        out = N.vpositions_array(n.value)
        off = np.zeros(g.value + 1, dtype=np.uint32)
        moves = np.zeros(n.value, dtype=np.uint16)
        end = np.zeros(n.value, dtype=np.uint8)
        N.check(N.lib.fnnue_build_vchildren(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off),
                                            len(games), N.ptr(out), len(out), N.ptr(off), len(off), N.ptr(moves),
                                            N.ptr(end), C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1], moves[: n.value], end[: n.value]

    def build_vchildren_device(self, variant: int, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int,
                               d_out: int, cap: int, d_off: int, off_cap: int, d_moves: int, d_end: int,
                               stream: int | None):
        """fnnue_build_vchildren_device -> (rc, records, groups); rc is FNNUE_E_CAPACITY (-10) on a sizing call."""
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_build_vchildren_device(self._h, variant, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                                C.c_void_p(d_moves_off), ngames, C.c_void_p(d_out), cap,
                                                C.c_void_p(d_off), off_cap, C.c_void_p(d_moves), C.c_void_p(d_end),
                                                C.byref(n), C.byref(g), C.c_void_p(stream))
        if rc != -10:
            N.check(rc)
        return rc, n.value, g.value

    def vsearch1(self, variant: int, games, cap: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_vsearch1: a one-ply search per ply of variant games -> (BEST_DTYPE records, CHAIN offsets).
        `cap` (default: the plies) sizes the record buffer."""
        text, fen_off, mv_off = pack_games(games)
        if cap is None:
            cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=BEST_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vsearch1(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                     N.ptr(out), cap, N.ptr(off), len(off), C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1]

    def vsearch1_device(self, variant: int, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, d_out: int,
                        cap: int, d_off: int, off_cap: int, stream: int | None) -> tuple[int, int]:
        """fnnue_vsearch1_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vsearch1_device(self._h, variant, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                            C.c_void_p(d_moves_off), ngames, C.c_void_p(d_out), cap, C.c_void_p(d_off),
                                            off_cap, C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    def vsearch1_lines(self, variant: int, games, k: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """fnnue_vsearch1_lines: vsearch1 plus each ply's k best children ->
        (BEST_DTYPE records, CHAIN offsets per game, LINE_DTYPE slots of shape (plies, k))."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=BEST_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        lines = np.zeros(max(cap * max(int(k), 0), 1), dtype=LINE_DTYPE)
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vsearch1_lines(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                           int(k), N.ptr(out), cap, N.ptr(off), len(off), N.ptr(lines), cap * int(k),
                                           C.byref(n), C.byref(g)))
        return out[: n.value], off[: g.value + 1], lines[: n.value * int(k)].reshape(n.value, int(k))

    def vsearch1_lines_device(self, variant: int, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, k: int,
                              d_out: int, cap: int, d_off: int, off_cap: int, d_lines: int, lines_cap: int,
                              stream: int | None) -> tuple[int, int]:
        """fnnue_vsearch1_lines_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when a buffer is too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vsearch1_lines_device(self._h, variant, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                                  C.c_void_p(d_moves_off), ngames, int(k), C.c_void_p(d_out), cap,
                                                  C.c_void_p(d_off), off_cap, C.c_void_p(d_lines), lines_cap,
                                                  C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    # The two-ply search of the variants (ABI 3.10)
    def vbest_replies(self, end, moves, off, child_best) -> np.ndarray:
        """fnnue_vbest_replies: best_replies with the variants' ranks (END_WON children, children whose
        every reply loses at once); kind may also be BEST_LOST."""
        end = np.ascontiguousarray(end, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        child_best = np.ascontiguousarray(child_best, dtype=BEST_DTYPE)
        if moves is not None:
            moves = np.ascontiguousarray(moves, dtype=np.uint16)
        out = np.zeros(len(off) - 1, dtype=BEST2_DTYPE)
        N.check(N.lib.fnnue_vbest_replies(self._h, N.ptr(end), N.ptr(moves), N.ptr(off), len(off) - 1, len(end),
                                          N.ptr(child_best), N.ptr(out)))
        return out

    def vbest_replies_device(self, d_end: int, d_moves: int | None, d_off: int, ngroups: int, npos: int,
                             d_child_best: int, d_out: int, stream: int | None):
        N.check(N.lib.fnnue_vbest_replies_device(self._h, C.c_void_p(d_end), C.c_void_p(d_moves), C.c_void_p(d_off),
                                                 ngroups, npos, C.c_void_p(d_child_best), C.c_void_p(d_out),
                                                 C.c_void_p(stream)))

    def vsearch2(self, variant: int, games, children: bool = False):
        """fnnue_vsearch2: a two-ply search per ply of variant games -> (BEST2_DTYPE records, CHAIN offsets).
        With `children` (fnnue_vsearch2_children) also the children's depth-1 records and their
        (ply, 1-based child index) pairs: -> (records, offsets, BEST_DTYPE records, (n, 2) uint32)."""
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        out = np.zeros(max(cap, 1), dtype=BEST2_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        if not children:
            N.check(N.lib.fnnue_vsearch2(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games),
                                         N.ptr(out), cap, N.ptr(off), len(off), C.byref(n), C.byref(g)))
            return out[: n.value], off[: g.value + 1]
        # a crazyhouse ply has no fixed child bound: the count comes back with FNNUE_E_CAPACITY
        nk = C.c_size_t()
        rc = N.lib.fnnue_vsearch2_children(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off),
                                           len(games), N.ptr(out), cap, N.ptr(off), len(off), None, None, 0,
                                           C.byref(n), C.byref(g), C.byref(nk))
        if rc != -10 or nk.value == 0:
            N.check(rc)
            return out[: n.value], off[: g.value + 1], np.zeros(0, dtype=BEST_DTYPE), np.zeros((0, 2), np.uint32)
        kcap = nk.value
        kb = np.zeros(kcap, dtype=BEST_DTYPE)
        km = np.zeros((kcap, 2), dtype=np.uint32)
        N.check(N.lib.fnnue_vsearch2_children(self._h, variant, text, len(text), N.ptr(fen_off), N.ptr(mv_off),
                                              len(games), N.ptr(out), cap, N.ptr(off), len(off), N.ptr(kb),
                                              N.ptr(km), kcap, C.byref(n), C.byref(g), C.byref(nk)))
        return out[: n.value], off[: g.value + 1], kb[: nk.value], km[: nk.value]

    def vsearch2_device(self, variant: int, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, d_out: int,
                        cap: int, d_off: int, off_cap: int, stream: int | None) -> tuple[int, int]:
        """fnnue_vsearch2_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when out / off are too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vsearch2_device(self._h, variant, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                            C.c_void_p(d_moves_off), ngames, C.c_void_p(d_out), cap, C.c_void_p(d_off),
                                            off_cap, C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    # MultiPV at two plies (ABI 3.11)
    def _topk_replies(self, fn, end, moves, off, child_best, k_or_line_off, lines_cap, fill):
        end = np.ascontiguousarray(end, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        child_best = np.ascontiguousarray(child_best, dtype=BEST_DTYPE)
        if moves is not None:
            moves = np.ascontiguousarray(moves, dtype=np.uint16)
        ng = len(off) - 1
        if np.ndim(k_or_line_off) == 0:
            line_off = (np.arange(ng + 1, dtype=np.uint64) * int(k_or_line_off)).astype(np.uint32)
        else:
            line_off = np.ascontiguousarray(k_or_line_off, dtype=np.uint32)
        cap = int(line_off[-1]) if lines_cap is None else int(lines_cap)
        lines = np.full(max(cap, 1) * N.LINE2_BYTES, fill, dtype=np.uint8).view(LINE2_DTYPE)
        N.check(fn(self._h, N.ptr(end), N.ptr(moves), N.ptr(off), ng, len(end), N.ptr(child_best), N.ptr(line_off),
                   N.ptr(lines), cap))
        return lines[:cap], line_off

    def topk_replies(self, end, moves, off, child_best, k_or_line_off, lines_cap: int | None = None,
                     fill: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_topk_replies: the k best lines of every STAR group from best_replies' arrays ->
        (LINE2_DTYPE slots, line_off).  `k_or_line_off`, `lines_cap` and `fill` as for topk_children."""
        return self._topk_replies(N.lib.fnnue_topk_replies, end, moves, off, child_best, k_or_line_off, lines_cap, fill)

    def vtopk_replies(self, end, moves, off, child_best, k_or_line_off, lines_cap: int | None = None,
                      fill: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """fnnue_vtopk_replies: topk_replies with the variants' ranks (vbest_replies' order)."""
        return self._topk_replies(N.lib.fnnue_vtopk_replies, end, moves, off, child_best, k_or_line_off, lines_cap,
                                  fill)

    def topk_replies_device(self, d_end: int, d_moves: int | None, d_off: int, ngroups: int, npos: int,
                            d_child_best: int, d_line_off: int, d_lines: int, lines_cap: int, stream: int | None):
        N.check(N.lib.fnnue_topk_replies_device(self._h, C.c_void_p(d_end), C.c_void_p(d_moves), C.c_void_p(d_off),
                                                ngroups, npos, C.c_void_p(d_child_best), C.c_void_p(d_line_off),
                                                C.c_void_p(d_lines), lines_cap, C.c_void_p(stream)))

    def vtopk_replies_device(self, d_end: int, d_moves: int | None, d_off: int, ngroups: int, npos: int,
                             d_child_best: int, d_line_off: int, d_lines: int, lines_cap: int, stream: int | None):
        N.check(N.lib.fnnue_vtopk_replies_device(self._h, C.c_void_p(d_end), C.c_void_p(d_moves), C.c_void_p(d_off),
                                                 ngroups, npos, C.c_void_p(d_child_best), C.c_void_p(d_line_off),
                                                 C.c_void_p(d_lines), lines_cap, C.c_void_p(stream)))

    def search2_lines(self, games, k: int, lines_cap: int | None = None):
        """fnnue_search2_lines: search2 plus each ply's k best lines ->
        (BEST2_DTYPE records, CHAIN offsets per game, LINE2_DTYPE slots of shape (plies, k)).
        `lines_cap` (default: plies * k) sizes the line buffer."""
        return self._search2_lines(None, games, k, lines_cap)

    def vsearch2_lines(self, variant: int, games, k: int, lines_cap: int | None = None):
        """fnnue_vsearch2_lines: vsearch2 plus each ply's k best lines (search2_lines' shapes)."""
        return self._search2_lines(int(variant), games, k, lines_cap)

    def _search2_lines(self, variant, games, k, lines_cap):
        text, fen_off, mv_off = pack_games(games)
        cap = sum(len((m if isinstance(m, str) else " ".join(m)).split()) + 1 for _, m in games)
        k = int(k)
        out = np.zeros(max(cap, 1), dtype=BEST2_DTYPE)
        off = np.zeros(len(games) + 1, dtype=np.uint32)
        lcap = cap * max(k, 0) if lines_cap is None else int(lines_cap)
        lines = np.zeros(max(lcap, 1), dtype=LINE2_DTYPE)
        n, g = C.c_size_t(), C.c_size_t()
        self.last_counts = (n, g)  # set also when the call is refused (FNNUE_E_CAPACITY)
        tail = (text, len(text), N.ptr(fen_off), N.ptr(mv_off), len(games), k, N.ptr(out), cap, N.ptr(off), len(off),
                N.ptr(lines), lcap, C.byref(n), C.byref(g))
        if variant is None:
            N.check(N.lib.fnnue_search2_lines(self._h, *tail))
        else:
            N.check(N.lib.fnnue_vsearch2_lines(self._h, variant, *tail))
        return out[: n.value], off[: g.value + 1], lines[: n.value * k].reshape(n.value, k)

    def search2_lines_device(self, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, k: int, d_out: int,
                             cap: int, d_off: int, off_cap: int, d_lines: int, lines_cap: int,
                             stream: int | None) -> tuple[int, int]:
        """fnnue_search2_lines_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when a buffer is too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_search2_lines_device(self._h, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                                 C.c_void_p(d_moves_off), ngames, int(k), C.c_void_p(d_out), cap,
                                                 C.c_void_p(d_off), off_cap, C.c_void_p(d_lines), lines_cap,
                                                 C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    def vsearch2_lines_device(self, variant: int, d_text: int, d_fen_off: int, d_moves_off: int, ngames: int, k: int,
                              d_out: int, cap: int, d_off: int, off_cap: int, d_lines: int, lines_cap: int,
                              stream: int | None) -> tuple[int, int]:
        """fnnue_vsearch2_lines_device -> (plies, games); FnnueError FNNUE_E_CAPACITY when a buffer is too small."""
        n, g = C.c_size_t(), C.c_size_t()
        N.check(N.lib.fnnue_vsearch2_lines_device(self._h, variant, C.c_void_p(d_text), C.c_void_p(d_fen_off),
                                                  C.c_void_p(d_moves_off), ngames, int(k), C.c_void_p(d_out), cap,
                                                  C.c_void_p(d_off), off_cap, C.c_void_p(d_lines), lines_cap,
                                                  C.byref(n), C.byref(g), C.c_void_p(stream)))
        return n.value, g.value

    def perft_device(self, fen: str, depth: int) -> int:
        nodes = C.c_uint64()
        N.check(N.lib.fnnue_perft_device(self._h, fen.encode(), depth, C.byref(nodes)))
        return nodes.value

    def set_ft_impl(self, impl: int) -> None:
        """FT_AUTO (default: gather for chess position calls of at most FT_GATHER_MAX positions,
        sliced otherwise and for every grouped call), FT_SLICED (LDS-stationary tiles) or
        FT_GATHER (per-position / per-group row gather)."""
        N.check(N.lib.fnnue_ctx_set_ft_impl(self._h, impl))

    def swar(self) -> tuple[bool, int]:
        """(SWAR row sums on, the net's accumulator bound)."""
        e, b = C.c_int(), C.c_int32()
        N.check(N.lib.fnnue_ctx_swar(self._h, C.byref(e), C.byref(b)))
        return bool(e.value), b.value

    def set_swar(self, enable: bool) -> None:
        N.check(N.lib.fnnue_ctx_set_swar(self._h, 1 if enable else 0))

    def swar_slices(self) -> tuple[int, int, int]:
        """(eligible, enabled, nslices): bit s of the masks is slice s (64 columns)."""
        el, en, ns = C.c_uint64(), C.c_uint64(), C.c_uint32()
        N.check(N.lib.fnnue_ctx_swar_slices(self._h, C.byref(el), C.byref(en), C.byref(ns)))
        return el.value, en.value, ns.value

    def set_swar_slices(self, mask: int) -> None:
        """Run SWAR rows in exactly the slices of `mask` (a subset of the eligible ones)."""
        N.check(N.lib.fnnue_ctx_set_swar_slices(self._h, mask))

    def set_timing(self, enable, ft_only: bool = False) -> None:
        """Events around every phase (plan / FT kernel / stacks), or with ft_only
        only the two around the FT main kernel (FNNUE_TIMING_FT: each event
        record costs the stream a few microseconds)."""
        N.check(N.lib.fnnue_ctx_set_timing(self._h, (N.TIMING_FT if ft_only else N.TIMING_ALL) if enable else N.TIMING_OFF))

    def timing_phases(self) -> tuple[int, float, float, float]:
        """(timed launches, summed ms of the FT plan kernels, of the FT main kernel, of the layer stacks); resets."""
        n, a, b, c = C.c_uint32(), C.c_double(), C.c_double(), C.c_double()
        N.check(N.lib.fnnue_ctx_timing_phases(self._h, C.byref(n), C.byref(a), C.byref(b), C.byref(c)))
        return n.value, a.value, b.value, c.value

    def timing_read(self) -> tuple[int, float, float]:
        """(timed launches, summed feature-transformer ms, summed layer-stack ms); resets."""
        n, a, b = C.c_uint32(), C.c_double(), C.c_double()
        N.check(N.lib.fnnue_ctx_timing_read(self._h, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            N.lib.fnnue_ctx_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        if N is not None and getattr(N, "lib", None) is not None:
            self.close()


class _BorrowedEvaluator(Evaluator):
    """The context of one device of a MultiEvaluator (owned by it)."""

    def __init__(self, handle: C.c_void_p, device: int):  # noqa: D401  (no ctx creation)
        self._h = handle
        self.device = device

    def close(self) -> None:
        self._h = C.c_void_p()


def _ptrs(vals) -> C.Array:
    return (C.c_void_p * len(vals))(*[C.c_void_p(v) for v in vals])


def _sizes(vals) -> C.Array:
    return (C.c_size_t * len(vals))(*vals)


def _streams(vals):
    return None if vals is None else _ptrs([v or 0 for v in vals])


class MultiEvaluator:
    """Several GPUs from one process (fnnue_multi_*): the net is RCCL-broadcast
    from devices[0]; batches are sharded without a data-path collective.  The
    reference's one-engine-per-core parallelism ([ref] src/main.rs:156-170).
    replicas=True (fnnue_multi_create_replicas): an ordinal may repeat and the
    image is copied to every context without RCCL, several contexts possibly
    on one GPU; every call after creation is the same."""

    def __init__(self, net: Net, devices, replicas: bool = False):
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        create = N.lib.fnnue_multi_create_replicas if replicas else N.lib.fnnue_multi_create
        N.check(create(net.handle, devs, len(devices), C.byref(h)))
        self._h = h
        self.devices = list(devices)

    def __len__(self) -> int:
        return len(self.devices)

    def ctx(self, i: int) -> Evaluator:
        h = C.c_void_p()
        N.check(N.lib.fnnue_multi_ctx(self._h, i, C.byref(h)))
        return _BorrowedEvaluator(h, self.devices[i])

    def eval_positions(self, pos: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        pos = np.ascontiguousarray(pos, dtype=np.uint8).reshape(-1, N.POS_BYTES)
        n = pos.shape[0]
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_multi_eval_positions(self._h, N.ptr(pos), n, N.ptr(psqt), N.ptr(positional)))
        return psqt, positional

    def eval_vpositions(self, vpos: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        vpos = np.ascontiguousarray(vpos, dtype=np.uint8).reshape(-1, N.VPOS_BYTES)
        n = vpos.shape[0]
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_multi_eval_vpositions(self._h, N.ptr(vpos), n, N.ptr(psqt), N.ptr(positional)))
        return psqt, positional

    def eval_groups(self, pos: np.ndarray, off: np.ndarray, mode: int = N.GROUP_CHAIN):
        pos = np.ascontiguousarray(pos, dtype=np.uint8).reshape(-1, N.POS_BYTES)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        if len(off) < 1 or int(off[-1]) != pos.shape[0]:
            raise ValueError("off must have >= 1 entry and end at the number of positions")
        n = pos.shape[0]
        psqt = np.zeros(n, dtype=np.int32)
        positional = np.zeros(n, dtype=np.int32)
        N.check(N.lib.fnnue_multi_eval_groups(self._h, N.ptr(pos), n, N.ptr(off), len(off) - 1, mode,
                                              N.ptr(psqt), N.ptr(positional)))
        return psqt, positional

    # device-resident shards: one pointer / count per device (asynchronous; then
    # sync()).  streams: one hipStream_t handle per device (e.g. torch's
    # current stream of each device) or None for the contexts' own streams.
    def eval_positions_device(self, d_pos, n, d_psqt, d_positional, streams=None) -> None:
        N.check(N.lib.fnnue_multi_eval_positions_device(self._h, _ptrs(d_pos), _sizes(n), _ptrs(d_psqt),
                                                        _ptrs(d_positional), _streams(streams)))

    def eval_vpositions_device(self, d_pos, n, d_psqt, d_positional, streams=None) -> None:
        N.check(N.lib.fnnue_multi_eval_vpositions_device(self._h, _ptrs(d_pos), _sizes(n), _ptrs(d_psqt),
                                                         _ptrs(d_positional), _streams(streams)))

    def eval_vgroups_device(self, d_pos, d_off, ngroups, npos, mode, d_psqt, d_positional, streams=None) -> None:
        N.check(N.lib.fnnue_multi_eval_vgroups_device(self._h, _ptrs(d_pos), _ptrs(d_off), _sizes(ngroups),
                                                      _sizes(npos), mode, _ptrs(d_psqt), _ptrs(d_positional),
                                                      _streams(streams)))

    def eval_groups_device(self, d_pos, d_off, ngroups, npos, mode, d_psqt, d_positional, streams=None) -> None:
        N.check(N.lib.fnnue_multi_eval_groups_device(self._h, _ptrs(d_pos), _ptrs(d_off), _sizes(ngroups),
                                                     _sizes(npos), mode, _ptrs(d_psqt), _ptrs(d_positional),
                                                     _streams(streams)))

    def sync(self) -> None:
        N.check(N.lib.fnnue_multi_sync(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            N.lib.fnnue_multi_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        if N is not None and getattr(N, "lib", None) is not None:
            self.close()


def partition_groups(off: np.ndarray, nparts: int) -> np.ndarray:
    """Whole groups into nparts contiguous runs of about equal position counts
    (fnnue_partition_groups): part k = groups [cut[k], cut[k + 1])."""
    off = np.ascontiguousarray(off, dtype=np.uint32)
    cut = np.zeros(nparts + 1, dtype=np.uint32)
    N.check(N.lib.fnnue_partition_groups(N.ptr(off), len(off) - 1, nparts, N.ptr(cut)))
    return cut


def pos_from_fen(fen: str) -> np.ndarray:
    out = N.positions_array(1)
    N.check(N.lib.fnnue_pos_from_fen(fen.encode(), N.ptr(out)))
    return out[0]


def game_positions(fen: str, moves: str | list[str]) -> np.ndarray:
    """Root + the position after every move (analysis batch expansion)."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    n = C.c_size_t()
    cap = moves.count(" ") + 2 if moves.strip() else 1
    out = N.positions_array(cap)
    N.check(N.lib.fnnue_game_positions(fen.encode(), moves.encode(), N.ptr(out), cap, C.byref(n)))
    return out[: n.value]


def game_children(fen: str, moves: str | list[str]) -> tuple[np.ndarray, np.ndarray]:
    """Every ply plus its legal 1-ply children, as STAR groups."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    nply = (moves.count(" ") + 2) if moves.strip() else 1
    cap = nply * 256
    out = N.positions_array(cap)
    off = np.zeros(nply + 1, dtype=np.uint32)
    n, g = C.c_size_t(), C.c_size_t()
    N.check(N.lib.fnnue_game_children(fen.encode(), moves.encode(), N.ptr(out), cap, N.ptr(off), len(off),
                                      C.byref(n), C.byref(g)))
    return out[: n.value], off[: g.value + 1]


def game_captures(fen: str, moves: str | list[str] = "") -> tuple[np.ndarray, np.ndarray]:
    """fnnue_game_captures: the game's last position followed by its capture children (legal moves after
    which the opponent has one piece fewer, in the order of game_children) -> (positions, uint16 move codes;
    codes[0] = 0)."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    cap = 128
    out = N.positions_array(cap)
    mv = np.zeros(cap, dtype=np.uint16)
    n = C.c_size_t()
    N.check(N.lib.fnnue_game_captures(fen.encode(), moves.encode(), N.ptr(out), cap, N.ptr(mv), C.byref(n)))
    return out[: n.value], mv[: n.value]


def game_quiet_moves(fen: str, moves: str | list[str] = "") -> tuple[np.ndarray, np.ndarray, bool]:
    """fnnue_game_quiet_moves: the game's last position followed by the candidates of the quiescence with
    checks (every legal move when the position is in check, its captures otherwise, in the order of
    game_children) -> (positions, uint16 move codes with codes[0] = 0, in check)."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    cap = 256
    out = N.positions_array(cap)
    mv = np.zeros(cap, dtype=np.uint16)
    n, chk = C.c_size_t(), C.c_int()
    N.check(N.lib.fnnue_game_quiet_moves(fen.encode(), moves.encode(), N.ptr(out), cap, N.ptr(mv), C.byref(chk),
                                         C.byref(n)))
    return out[: n.value], mv[: n.value], bool(chk.value)


VQ_CHECK, VQ_LOST, VQ_WON, VQ_DRAWN = 1, 2, 4, 8  # FNNUE_VQ_*: game_vquiet_moves' state bits


def game_vquiet_moves(variant: int, fen: str, moves: str | list[str] = "",
                      checks: bool = False) -> tuple[np.ndarray, np.ndarray, int]:
    """fnnue_game_vquiet_moves: the variant game's last position followed by the candidates of the variants'
    quiescence (every legal move, drops included, when `checks` and the position is in check; its captures
    otherwise; nothing when the game is over) -> (positions, uint16 variant move codes with codes[0] = 0,
    VQ_* state bits)."""
    if not isinstance(moves, str):
        moves = " ".join(moves)
    n, state = C.c_size_t(), C.c_int()
    rc = N.lib.fnnue_game_vquiet_moves(variant, fen.encode(), moves.encode(), 1 if checks else 0, None, 0, None,
                                       C.byref(state), C.byref(n))
    if rc != -10:
        N.check(rc)
    cap = n.value
    out = N.vpositions_array(cap)
    mv = np.zeros(cap, dtype=np.uint16)
    N.check(N.lib.fnnue_game_vquiet_moves(variant, fen.encode(), moves.encode(), 1 if checks else 0, N.ptr(out), cap,
                                          N.ptr(mv), C.byref(state), C.byref(n)))
    return out[: n.value], mv[: n.value], state.value


def random_playouts(seed: int, count: int, min_plies: int = 0, max_plies: int = 160,
                    mode: int = N.PLAYOUT_FINAL, threads: int = 8, cap: int | None = None):
    """Seeded random-playout positions.  FINAL -> positions;
    PLIES / CHILDREN -> (positions, group offsets)."""
    if cap is None:
        per = {N.PLAYOUT_FINAL: 1, N.PLAYOUT_PLIES: max_plies + 1, N.PLAYOUT_CHILDREN: (max_plies + 1) * 40}[mode]
        cap = count * per
    offcap = count * (max_plies + 1) + 1 if mode != N.PLAYOUT_FINAL else 1
    for _ in range(2):
        out = N.positions_array(cap)
        off = np.zeros(offcap, dtype=np.uint32)
        n, g = C.c_size_t(), C.c_size_t()
        rc = N.lib.fnnue_random_playouts(seed, count, min_plies, max_plies, mode, threads, N.ptr(out), cap,
                                         N.ptr(off), len(off), C.byref(n), C.byref(g))
        if rc == -10 and n.value > cap:  # FNNUE_E_CAPACITY: retry with the exact size
            cap = n.value
            continue
        N.check(rc)
        break
    if mode == N.PLAYOUT_FINAL:
        return out[: n.value]
    return out[: n.value], off[: g.value + 1]


def pack_games(games) -> tuple[bytes, np.ndarray, np.ndarray]:
    """[(fen, moves)] -> the builder's text layout: FEN g in [fen_off[g], mv_off[g]),
    its moves in [mv_off[g], fen_off[g + 1])."""
    parts, fen_off, mv_off, pos = [], [], [], 0
    for fen, moves in games:
        if not isinstance(moves, str):
            moves = " ".join(moves)
        f, m = fen.encode(), b" " + moves.encode()
        fen_off.append(pos)
        mv_off.append(pos + len(f))
        parts += [f, m]
        pos += len(f) + len(m)
    fen_off.append(pos)
    return b"".join(parts), np.array(fen_off, dtype=np.uint32), np.array(mv_off, dtype=np.uint32)


def random_game(seed: int, fen: str, plies: int) -> str:
    """Up to `plies` random legal moves from `fen` as space-separated UCI (test inputs)."""
    n = C.c_size_t()
    buf = C.create_string_buffer(8 * plies + 16)
    N.check(N.lib.fnnue_random_game(seed, fen.encode(), plies, buf, len(buf), C.byref(n)))
    return buf.value.decode()


def perft(fen: str, depth: int) -> int:
    nodes = C.c_uint64()
    N.check(N.lib.fnnue_perft(fen.encode(), depth, C.byref(nodes)))
    return nodes.value


def selftest_mfma(device: int = 0) -> None:
    N.check(N.lib.fnnue_selftest_mfma(device))

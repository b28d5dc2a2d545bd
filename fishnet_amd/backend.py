"""fnnue_backend (include/fnnue_backend.h) in Python: fishnet's engine-actor
shape over the GPU evaluator.

Mirrors the reference's interface for this path:
  ``stockfish::channel(exe, init, logger) -> (StockfishStub, StockfishActor)``
  ([ref] src/stockfish.rs:23-38) and ``StockfishStub::go(Position) ->
  Result<PositionResponse, PositionFailed>`` (:44-54), with
  ``AcquireResponseBody`` (src/api.rs:293-309), ``PositionResponse`` /
  ``PositionFailed`` (src/ipc.rs:28-39, 100-103), ``Score`` (api.rs:383-388)
  and ``CompletedBatch::into_analysis`` (src/queue.rs:715-727).
Here ``go`` takes whole acquired batches (the GPU wants batches, not single
positions) and returns, per batch, its responses or a ``PositionFailed``.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from . import _native as N
from .nnue import vmove_uci

WORK_ANALYSIS, WORK_MOVE = 0, 1
SCORE_CP, SCORE_MATE = 0, 1


class _Init(C.Structure):
    _fields_ = [("normalize_to_pawn", C.c_int32), ("timeout_ms", C.c_uint32)]


class _Acquired(C.Structure):
    _fields_ = [("batch_id", C.c_char_p), ("work", C.c_int), ("multipv", C.c_int), ("position", C.c_char_p),
                ("variant", C.c_char_p), ("moves", C.c_char_p), ("skip_positions", C.c_void_p),
                ("nskip", C.c_size_t)]


class _Response(C.Structure):
    _fields_ = [("position_id", C.c_uint32), ("skipped", C.c_uint8), ("score_kind", C.c_uint8),
                ("depth", C.c_uint8), ("matrix", C.c_uint8), ("score", C.c_int64), ("psqt", C.c_int32),
                ("positional", C.c_int32), ("nodes", C.c_uint64), ("time_ms", C.c_uint64), ("nps", C.c_uint32),
                ("best_move", C.c_char * 8)]


class _PvLine(C.Structure):
    _fields_ = [("score", C.c_int64), ("psqt", C.c_int32), ("positional", C.c_int32), ("move", C.c_char * 7),
                ("score_kind", C.c_uint8)]


class _PvLine2(C.Structure):
    _fields_ = [("score", C.c_int64), ("psqt", C.c_int32), ("positional", C.c_int32), ("pv", C.c_char * 14),
                ("score_kind", C.c_uint8), ("pv_len", C.c_uint8)]


class _Compact(C.Structure):
    _fields_ = [("psqt", C.c_int32), ("positional", C.c_int32), ("score", C.c_int32), ("score_kind", C.c_uint8),
                ("depth", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8)]


class _BatchCompact(C.Structure):
    _fields_ = [("time_ms", C.c_uint64), ("nps", C.c_uint32), ("nodes", C.c_uint32), ("best_move", C.c_char * 8)]


COMPACT_SKIPPED, COMPACT_MATRIX, COMPACT_NO_MOVES = 1, 2, 4


@dataclass
class AcquireResponseBody:
    """One acquired batch: work type + id, root FEN, variant, UCI moves, skipPositions."""
    batch_id: str
    position: str
    moves: str | Sequence[str] = ""
    work: str = "analysis"            # "analysis" | "move"
    variant: str = "standard"
    skip_positions: Sequence[int] = ()
    multipv: int | None = None


@dataclass
class Score:
    kind: str   # "cp" | "mate"
    value: int


@dataclass
class PvLine:
    """One MultiPV line of a response (fnnue_pv_line): its score and its pv, one move."""
    score: Score
    move: str
    psqt: int = 0
    positional: int = 0


@dataclass
class PvLine2:
    """One MultiPV line with its whole pv (fnnue_pv_line2): `pv` holds one or two UCI moves."""
    score: Score
    pv: list[str]
    psqt: int = 0
    positional: int = 0


@dataclass
class PositionResponse:
    position_id: int
    score: Score | None               # None for Skip::Skip
    psqt: int = 0
    positional: int = 0
    depth: int = 0
    nodes: int = 0
    time_ms: int = 0
    nps: int = 0
    best_move: str | None = None
    skipped: bool = False
    matrix: bool = False              # AnalysisPart::Matrix (the batch asked for multipv)
    # go_lines: the MultiPV lines, best first (None: go() / no line); go_lines_pv: PvLine2 lines
    lines: list[PvLine] | list[PvLine2] | None = None
    reply: str | None = None          # go_pv on a 2-plies channel: the pv's second move (None: no reply)


@dataclass
class PositionFailed(Exception):
    batch_id: str
    code: int = 0
    message: str = field(default="")

    def __str__(self) -> str:
        return f"PositionFailed({self.batch_id}): {N.ERRORS.get(self.code, self.code)} {self.message}"


def batch_size(body: AcquireResponseBody) -> int:
    """Responses the batch expands to (IncomingBatch::from_acquired): moves + 1, or 1 for move work."""
    a, _keep = _acquired([body])
    n = C.c_size_t()
    N.check(N.lib.fnnue_backend_batch_size(C.byref(a[0]), C.byref(n)))
    return n.value


def lines_bound(bodies: Sequence[AcquireResponseBody]) -> int:
    """fnnue_backend_lines_bound: the lines a go_lines() over these batches may write."""
    a, _keep = _acquired(bodies)
    n = C.c_size_t()
    N.check(N.lib.fnnue_backend_lines_bound(a, len(bodies), C.byref(n)))
    return n.value


def _acquired(bodies: Sequence[AcquireResponseBody]):
    arr = (_Acquired * max(1, len(bodies)))()
    keep = []
    for i, b in enumerate(bodies):
        moves = b.moves if isinstance(b.moves, str) else " ".join(b.moves)
        skip = np.ascontiguousarray(np.asarray(list(b.skip_positions), dtype=np.uint32))
        keep.append(skip)
        strs = [s.encode() for s in (b.batch_id, b.position, b.variant or "", moves)]
        keep += strs
        work = {"analysis": WORK_ANALYSIS, "move": WORK_MOVE}.get(b.work, -1)
        arr[i] = _Acquired(strs[0], work, int(b.multipv or 0), strs[1], strs[2], strs[3],
                           skip.ctypes.data if len(skip) else None, len(skip))
    return arr, keep


class GpuEvalActor:
    """The actor half: owns the worker thread and the evaluator (fnnue_backend)."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            N.lib.fnnue_backend_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        if N is not None and getattr(N, "lib", None) is not None:
            self.close()


class GpuEvalStub:
    """StockfishStub for the GPU backend: ``go`` sends batches over the channel."""

    def __init__(self, actor: GpuEvalActor):
        self._actor = actor

    def go(self, bodies: Sequence[AcquireResponseBody],
           timeout_ms: int = 0) -> list[list[PositionResponse] | PositionFailed]:
        """One go() over whole batches, within `timeout_ms` (0: the channel's
        budget).  A call that overruns it raises FnnueError FNNUE_E_TIMEOUT and
        breaks the channel (fnnue_backend_go_timeout); `last_batch_rc` then
        says which batches had been answered."""
        return self._go(bodies, timeout_ms, None)

    def go_lines(self, bodies: Sequence[AcquireResponseBody], timeout_ms: int = 0,
                 lines_cap: int | None = None) -> list[list[PositionResponse] | PositionFailed]:
        """go() with the MultiPV lines (fnnue_backend_go_lines): on a depth-1
        channel (for variant batches: variant_analysis_depth 1) every
        non-skipped ply with a legal move of an analysis
        batch with multipv = k carries `lines`, its min(k, nodes) best moves,
        best first; every other response has lines = None.  `lines_cap`: the
        line buffer's size (default: lines_bound(bodies))."""
        return self._go(bodies, timeout_ms, lines_bound(bodies) if lines_cap is None else int(lines_cap))

    def go_pv(self, bodies: Sequence[AcquireResponseBody],
              timeout_ms: int = 0) -> list[list[PositionResponse] | PositionFailed]:
        """go() with the pv's second move (fnnue_backend_go_pv): on a 2-plies
        channel every ply whose pv has two moves carries `reply`; every other
        response has reply = None."""
        return self._go(bodies, timeout_ms, None, with_reply=True)

    def go_lines_pv(self, bodies: Sequence[AcquireResponseBody], timeout_ms: int = 0,
                    lines_cap: int | None = None) -> list[list[PositionResponse] | PositionFailed]:
        """go_pv() with the MultiPV lines and their whole pvs (fnnue_backend_go_lines_pv): the rows and
        their `reply` are go_pv()'s; on a 2-plies setting every non-skipped ply with a legal move of an
        analysis batch with multipv = k carries `lines`, its min(k, legal moves) best PvLine2 lines
        (`pv`: one or two UCI moves), best first; on a 1-ply setting go_lines' lines as one-move
        PvLine2; every other response has lines = None."""
        return self._go(bodies, timeout_ms, lines_bound(bodies) if lines_cap is None else int(lines_cap),
                        with_reply=True, pv2=True)

    def _go(self, bodies, timeout_ms, lines_cap, with_reply=False, pv2=False):
        nb = len(bodies)
        if nb == 0:
            return []
        a, _keep = _acquired(bodies)
        cap = 0
        for b in bodies:
            moves = b.moves if isinstance(b.moves, str) else " ".join(b.moves)
            cap += 1 if b.work == "move" else len(moves.split()) + 1
        out = (_Response * max(1, cap))()
        off = np.zeros(nb + 1, dtype=np.uint32)
        rc = np.zeros(nb, dtype=np.int32)
        self.last_batch_rc = rc
        t0 = time.perf_counter()
        if pv2:
            reply = np.zeros(max(1, cap), dtype=np.uint16)
            pv = (_PvLine2 * max(1, lines_cap))()
            loff = np.zeros(cap + 1, dtype=np.uint32)
            t0 = time.perf_counter()
            ret = N.lib.fnnue_backend_go_lines_pv(self._actor._h, a, nb, out, cap, N.ptr(off), N.ptr(rc), pv, lines_cap,
                                                  N.ptr(loff), N.ptr(reply), int(timeout_ms))
        elif with_reply:
            reply = np.zeros(max(1, cap), dtype=np.uint16)
            ret = N.lib.fnnue_backend_go_pv(self._actor._h, a, nb, out, cap, N.ptr(off), N.ptr(rc), N.ptr(reply),
                                            int(timeout_ms))
        elif lines_cap is None:
            ret = N.lib.fnnue_backend_go_timeout(self._actor._h, a, nb, out, cap, N.ptr(off), N.ptr(rc),
                                                 int(timeout_ms))
        else:
            pv = (_PvLine * max(1, lines_cap))()
            loff = np.zeros(cap + 1, dtype=np.uint32)
            t0 = time.perf_counter()
            ret = N.lib.fnnue_backend_go_lines(self._actor._h, a, nb, out, cap, N.ptr(off), N.ptr(rc), pv, lines_cap,
                                               N.ptr(loff), int(timeout_ms))
        self.last_call_s = time.perf_counter() - t0  # the C call alone (not the ctypes marshalling around it)
        N.check(ret)
        res: list[list[PositionResponse] | PositionFailed] = []
        for i, b in enumerate(bodies):
            if rc[i]:
                res.append(PositionFailed(b.batch_id, int(rc[i])))
                continue
            rows = []
            for k in range(int(off[i]), int(off[i + 1])):
                r = out[k]
                if r.skipped:
                    rows.append(PositionResponse(r.position_id, None, skipped=True))
                    continue
                rows.append(PositionResponse(
                    r.position_id, Score("mate" if r.score_kind == SCORE_MATE else "cp", int(r.score)), r.psqt,
                    r.positional, r.depth, r.nodes, r.time_ms, r.nps, r.best_move.decode() or None,
                    matrix=bool(r.matrix)))
                if with_reply and reply[k]:
                    rows[-1].reply = vmove_uci(int(reply[k]))  # a chess code prints as move_uci prints it
                if pv2 and loff[k + 1] > loff[k]:
                    rows[-1].lines = [
                        PvLine2(Score("mate" if l.score_kind == SCORE_MATE else "cp", int(l.score)),
                                l.pv.decode().split(), l.psqt, l.positional)
                        for l in pv[int(loff[k]):int(loff[k + 1])]]
                elif lines_cap is not None and loff[k + 1] > loff[k]:
                    rows[-1].lines = [
                        PvLine(Score("mate" if l.score_kind == SCORE_MATE else "cp", int(l.score)), l.move.decode(),
                               l.psqt, l.positional) for l in pv[int(loff[k]):int(loff[k + 1])]]
            res.append(rows)
        return res

    def go_compact(self, bodies: Sequence[AcquireResponseBody],
                   timeout_ms: int = 0) -> list[list[PositionResponse] | PositionFailed]:
        """go() through the compact form (fnnue_backend_go_compact: 16 B per
        position + 24 B per batch), expanded here into the same
        PositionResponses the full form gives."""
        nb = len(bodies)
        if nb == 0:
            return []
        a, _keep = _acquired(bodies)
        cap = sum(1 if b.work == "move" else len((b.moves if isinstance(b.moves, str) else " ".join(b.moves)).split()) + 1
                  for b in bodies)
        out = (_Compact * max(1, cap))()
        bout = (_BatchCompact * nb)()
        off = np.zeros(nb + 1, dtype=np.uint32)
        rc = np.zeros(nb, dtype=np.int32)
        self.last_batch_rc = rc
        t0 = time.perf_counter()
        ret = N.lib.fnnue_backend_go_compact(self._actor._h, a, nb, out, cap, bout, N.ptr(off), N.ptr(rc),
                                             int(timeout_ms))
        self.last_call_s = time.perf_counter() - t0
        N.check(ret)
        res: list[list[PositionResponse] | PositionFailed] = []
        for i, b in enumerate(bodies):
            if rc[i]:
                res.append(PositionFailed(b.batch_id, int(rc[i])))
                continue
            bt = bout[i]
            rows = []
            for k in range(int(off[i]), int(off[i + 1])):
                r = out[k]
                pid = k - int(off[i])
                if r.flags & COMPACT_SKIPPED:
                    rows.append(PositionResponse(pid, None, skipped=True))
                    continue
                move = b.work == "move"
                nodes = 0 if r.flags & COMPACT_NO_MOVES else (bt.nodes if move else 1)
                rows.append(PositionResponse(
                    pid, Score("mate" if r.score_kind == SCORE_MATE else "cp", int(r.score)), r.psqt, r.positional,
                    r.depth, nodes, bt.time_ms, bt.nps, (bt.best_move.decode() or None) if move else None,
                    matrix=bool(r.flags & COMPACT_MATRIX)))
            res.append(rows)
        return res

    def set_analysis_depth(self, depth: int) -> None:
        """fnnue_backend_set_analysis_depth: 0 = a static evaluation per ply (the
        default), 1 = a one-ply search per chess analysis ply (best move, pv)."""
        N.check(N.lib.fnnue_backend_set_analysis_depth(self._actor._h, int(depth)))

    def set_analysis_plies(self, plies: int) -> None:
        """fnnue_backend_set_analysis_plies: 0 and 1 as set_analysis_depth, 2 = a full-width two-ply
        search per chess analysis ply (best move, the reply in go_pv's rows)."""
        N.check(N.lib.fnnue_backend_set_analysis_plies(self._actor._h, int(plies)))

    def set_variant_analysis_depth(self, depth: int) -> None:
        """fnnue_backend_set_variant_analysis_depth: the same for crazyhouse, atomic, kingOfTheHill,
        racingKings and threeCheck analysis batches (drops as "N@f3"); independent of set_analysis_depth."""
        N.check(N.lib.fnnue_backend_set_variant_analysis_depth(self._actor._h, int(depth)))

    def set_variant_analysis_plies(self, plies: int) -> None:
        """fnnue_backend_set_variant_analysis_plies: 0 and 1 as set_variant_analysis_depth, 2 = a two-ply
        search per variant analysis ply under the variant's rules (the reply in go_pv's rows, drops included)."""
        N.check(N.lib.fnnue_backend_set_variant_analysis_plies(self._actor._h, int(plies)))

    def set_draw_rules(self, on: bool) -> None:
        """fnnue_backend_set_draw_rules: chess analysis batches at 1 or 2 plies score the moves that repeat a
        position for the third time or reach the fifty-move rule as draws (Cp 0, the pv ends there)."""
        N.check(N.lib.fnnue_backend_set_draw_rules(self._actor._h, 1 if on else 0))

    def draw_rules(self) -> bool:
        on = C.c_int()
        N.check(N.lib.fnnue_backend_draw_rules(self._actor._h, C.byref(on)))
        return bool(on.value)

    def set_quiesce(self, depth: int) -> None:
        """fnnue_backend_set_quiesce: chess analysis batches at 1 or 2 plies resolve captures below their leaves,
        `depth` captures deep at most (0: off; fnnue.h has the rule)."""
        N.check(N.lib.fnnue_backend_set_quiesce(self._actor._h, int(depth)))

    def quiesce(self) -> int:
        d = C.c_int()
        N.check(N.lib.fnnue_backend_quiesce(self._actor._h, C.byref(d)))
        return d.value

    def set_quiesce_checks(self, on: bool) -> None:
        """fnnue_backend_set_quiesce_checks: the quiescence of chess analysis batches recognises check evasions
        and mates (fnnue.h: Q'), and coded mate values are answered as Score::Mate."""
        N.check(N.lib.fnnue_backend_set_quiesce_checks(self._actor._h, 1 if on else 0))

    def quiesce_checks(self) -> bool:
        on = C.c_int()
        N.check(N.lib.fnnue_backend_quiesce_checks(self._actor._h, C.byref(on)))
        return bool(on.value)

    def set_variant_quiesce(self, depth: int, checks: bool = False) -> None:
        """fnnue_backend_set_variant_quiesce: variant analysis batches at 1 or 2 plies resolve captures below their
        leaves under the variant's rule, `depth` deep at most (0: off); `checks`: evasions and mates inside it.
        With a depth set, coded mates are answered as Score::Mate."""
        N.check(N.lib.fnnue_backend_set_variant_quiesce(self._actor._h, int(depth), 1 if checks else 0))

    def variant_quiesce(self) -> tuple[int, bool]:
        d, on = C.c_int(), C.c_int()
        N.check(N.lib.fnnue_backend_variant_quiesce(self._actor._h, C.byref(d), C.byref(on)))
        return d.value, bool(on.value)

    def set_variant_draw_rules(self, on: bool) -> None:
        """fnnue_backend_set_variant_draw_rules: variant analysis batches at 1 or 2 plies score the moves that
        repeat a position for the third time, or reach the clock rule of their variant, as draws (fnnue.h, ABI
        3.16; Cp 0, the pv ends there).  Chess batches keep following set_draw_rules."""
        N.check(N.lib.fnnue_backend_set_variant_draw_rules(self._actor._h, 1 if on else 0))

    def variant_draw_rules(self) -> bool:
        on = C.c_int()
        N.check(N.lib.fnnue_backend_variant_draw_rules(self._actor._h, C.byref(on)))
        return bool(on.value)

    def go_one(self, body: AcquireResponseBody) -> list[PositionResponse]:
        """One batch; raises PositionFailed like StockfishStub::go's Err."""
        r = self.go([body])[0]
        if isinstance(r, PositionFailed):
            raise r
        return r


class _Stats(C.Structure):
    _fields_ = [("prep_ms", C.c_double), ("device_ms", C.c_double), ("fill_ms", C.c_double), ("total_ms", C.c_double),
                ("positions", C.c_uint64), ("stream_syncs", C.c_uint32), ("rebuilds", C.c_uint32),
                ("host_threads", C.c_uint32), ("pieces", C.c_uint32)]


def last_stats(actor: "GpuEvalActor") -> dict:
    """fnnue_backend_last_stats: where the last go() spent its time."""
    st = _Stats()
    N.check(N.lib.fnnue_backend_last_stats(actor._h, C.byref(st)))
    return {k: getattr(st, k) for k, _ in _Stats._fields_}


class _Nets(C.Structure):
    _fields_ = [("chess", C.c_void_p), ("crazyhouse", C.c_void_p), ("atomic", C.c_void_p)]


def channel(net=None, device: int = 0, normalize_to_pawn: int = 0, *, crazyhouse=None,
            atomic=None, kingofthehill=None, racingkings=None, threecheck=None, timeout_ms: int = 0,
            analysis_depth: int = 0, variant_analysis_depth: int = 0,
            analysis_plies: int | None = None,
            variant_analysis_plies: int | None = None,
            draw_rules: bool = False, quiesce: int = 0,
            quiesce_checks: bool = False, variant_quiesce: int = 0,
            variant_quiesce_checks: bool = False,
            variant_draw_rules: bool = False) -> tuple[GpuEvalStub, GpuEvalActor]:
    """stockfish::channel for the GPU evaluator.  `net` (a fishnet_amd.Net)
    goes to the slot of its variant; `crazyhouse` / `atomic` add variant nets
    (fnnue_backend_channel_nets), `kingofthehill` / `racingkings` / `threecheck` theirs
    (fnnue_backend_channel_netv): each batch is evaluated by its variant's net.
    `timeout_ms`: the budget of each go() (0: 60 s, [ref] src/main.rs:316).
    `analysis_depth`: 0 or 1 (GpuEvalStub.set_analysis_depth); `variant_analysis_depth`: 0 or 1
    for the variant nets' batches (GpuEvalStub.set_variant_analysis_depth); `analysis_plies`: 0, 1 or 2
    (GpuEvalStub.set_analysis_plies; it takes the place of `analysis_depth`); `variant_analysis_plies`: 0, 1
    or 2 for the variant nets' batches (GpuEvalStub.set_variant_analysis_plies; it takes the place of
    `variant_analysis_depth`); `draw_rules`: repetition and fifty-move draws in the chess searches
    (GpuEvalStub.set_draw_rules; off by default); `quiesce`: the capture quiescence depth below the chess
    searches' leaves (GpuEvalStub.set_quiesce; 0 by default); `quiesce_checks`: check evasions and mates inside
    that quiescence (GpuEvalStub.set_quiesce_checks; off by default); `variant_quiesce` /
    `variant_quiesce_checks`: the same for the variant nets' batches under the variants' rule
    (GpuEvalStub.set_variant_quiesce; 0 / off by default); `variant_draw_rules`: repetition and n-move draws in
    the variant searches, each variant's own rule (GpuEvalStub.set_variant_draw_rules; off by default)."""
    h = C.c_void_p()
    init = _Init(normalize_to_pawn, timeout_ms)
    if kingofthehill is not None or racingkings is not None or threecheck is not None:
        given = [n for n in (net, crazyhouse, atomic, kingofthehill, racingkings, threecheck) if n is not None]
        arr = (C.c_void_p * len(given))(*[n._h.value for n in given])
        N.check(N.lib.fnnue_backend_channel_netv(arr, len(given), device, C.byref(init), C.byref(h)))
    elif crazyhouse is None and atomic is None:
        N.check(N.lib.fnnue_backend_channel(net._h, device, C.byref(init), C.byref(h)))
    else:
        nets = _Nets(net._h if net is not None else None, crazyhouse._h if crazyhouse is not None else None,
                     atomic._h if atomic is not None else None)
        N.check(N.lib.fnnue_backend_channel_nets(C.byref(nets), device, C.byref(init), C.byref(h)))
    actor = GpuEvalActor(h)
    stub = GpuEvalStub(actor)
    if analysis_depth:
        stub.set_analysis_depth(analysis_depth)
    if variant_analysis_depth:
        stub.set_variant_analysis_depth(variant_analysis_depth)
    if analysis_plies is not None:
        stub.set_analysis_plies(analysis_plies)
    if variant_analysis_plies is not None:
        stub.set_variant_analysis_plies(variant_analysis_plies)
    if draw_rules:
        stub.set_draw_rules(True)
    if quiesce:
        stub.set_quiesce(quiesce)
    if quiesce_checks:
        stub.set_quiesce_checks(True)
    if variant_quiesce or variant_quiesce_checks:
        stub.set_variant_quiesce(variant_quiesce, variant_quiesce_checks)
    if variant_draw_rules:
        stub.set_variant_draw_rules(True)
    return stub, actor


def _move_code(uci: str | None) -> int:
    """The fnnue_move code of a move's UCI text (0 for None / ""); a variant's drop "N@f3" is
    from == to with the piece type in the promotion field (fnnue_vmove_uci)."""
    if not uci:
        return 0
    sq = lambda s: (ord(s[0]) - 97) | (int(s[1]) - 1) << 3
    if uci[1] == "@":
        return sq(uci[2:4]) | sq(uci[2:4]) << 6 | " PNBRQ".index(uci[0].upper()) << 12
    return sq(uci[0:2]) | sq(uci[2:4]) << 6 | (" pnbrq".index(uci[4]) if len(uci) > 4 else 0) << 12


def into_analysis(responses: Sequence[PositionResponse]) -> str:
    """The `analysis` JSON array of a completed analysis batch (fnnue_backend_analysis_json; with
    MultiPV lines, fnnue_backend_analysis_json_lines, or for go_lines_pv's PvLine2 lines
    fnnue_backend_analysis_json_lines_pv; with a row's `reply`, the two-move pv of
    fnnue_backend_analysis_json_pv)."""
    arr = (_Response * max(1, len(responses)))()
    for i, r in enumerate(responses):
        if r.skipped:
            arr[i] = _Response(r.position_id, 1)
            continue
        kind = SCORE_MATE if r.score.kind == "mate" else SCORE_CP
        arr[i] = _Response(r.position_id, 0, kind, r.depth, 1 if r.matrix else 0, r.score.value, r.psqt,
                           r.positional, r.nodes, r.time_ms, r.nps, (r.best_move or "").encode())
    n = C.c_size_t()
    if any(isinstance(l, PvLine2) for r in responses for l in r.lines or ()):  # go_lines_pv rows: whole pvs
        loff = np.zeros(len(responses) + 1, dtype=np.uint32)
        loff[1:] = np.cumsum([len(r.lines or ()) for r in responses])
        pv2 = (_PvLine2 * max(1, int(loff[-1])))()
        at = 0
        for r in responses:
            for l in r.lines or ():
                pv2[at] = _PvLine2(l.score.value, l.psqt, l.positional, " ".join(l.pv).encode(),
                                   SCORE_MATE if l.score.kind == "mate" else SCORE_CP, len(l.pv))
                at += 1
        N.lib.fnnue_backend_analysis_json_lines_pv(arr, len(responses), pv2, N.ptr(loff), None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value + 1)
        N.check(N.lib.fnnue_backend_analysis_json_lines_pv(arr, len(responses), pv2, N.ptr(loff), buf, len(buf),
                                                           C.byref(n)))
        return buf.value.decode()
    if any(r.lines for r in responses):  # MultiPV: the matrix with one row per line
        loff = np.zeros(len(responses) + 1, dtype=np.uint32)
        loff[1:] = np.cumsum([len(r.lines or ()) for r in responses])
        pv = (_PvLine * max(1, int(loff[-1])))()
        at = 0
        for r in responses:
            for l in r.lines or ():
                pv[at] = _PvLine(l.score.value, l.psqt, l.positional, l.move.encode(),
                                 SCORE_MATE if l.score.kind == "mate" else SCORE_CP)
                at += 1
        N.lib.fnnue_backend_analysis_json_lines(arr, len(responses), pv, N.ptr(loff), None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value + 1)
        N.check(N.lib.fnnue_backend_analysis_json_lines(arr, len(responses), pv, N.ptr(loff), buf, len(buf),
                                                        C.byref(n)))
        return buf.value.decode()
    if any(getattr(r, "reply", None) for r in responses):  # go_pv rows: the pv's second move
        reply = np.array([_move_code(getattr(r, "reply", None)) for r in responses], dtype=np.uint16)
        N.lib.fnnue_backend_analysis_json_pv(arr, len(responses), N.ptr(reply), None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value + 1)
        N.check(N.lib.fnnue_backend_analysis_json_pv(arr, len(responses), N.ptr(reply), buf, len(buf), C.byref(n)))
        return buf.value.decode()
    N.lib.fnnue_backend_analysis_json(arr, len(responses), None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value + 1)
    N.check(N.lib.fnnue_backend_analysis_json(arr, len(responses), buf, len(buf), C.byref(n)))
    return buf.value.decode()

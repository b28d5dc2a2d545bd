"""The host side of MultiPV at analysis depth 1 (ABI 3.5): the layouts of
fnnue_line and fnnue_pv_line, the no-device error paths of the new entry
points, fnnue_backend_lines_bound on hand-made bodies, and the `analysis` JSON
with k rows per matrix (Matrix::set per line, [ref] src/ipc.rs:77-86) against
literal strings."""
import ctypes as C

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B

E_ARG, E_CAPACITY = -1, -10


def test_line_record_layout():
    assert C.sizeof(F.Line) == 20 and N.LINE_BYTES == 20 and F.LINE_DTYPE.itemsize == 20
    assert [(n, F.LINE_DTYPE.fields[n][1]) for n in F.LINE_DTYPE.names] == \
        [(n, getattr(F.Line, n).offset) for n, _ in F.Line._fields_]
    assert (F.Line.child.offset, F.Line.move.offset, F.Line.kind.offset, F.Line.reserved.offset) == (12, 16, 18, 19)
    assert F.MAX_CHILDREN == 218


def test_pv_line_layout():
    assert C.sizeof(B._PvLine) == 24 and N.PV_LINE_BYTES == 24
    assert (B._PvLine.score.offset, B._PvLine.psqt.offset, B._PvLine.positional.offset) == (0, 8, 12)
    assert (B._PvLine.move.offset, B._PvLine.score_kind.offset) == (16, 23)
    assert C.sizeof(B._Response) == 56  # the response record did not grow


def test_abi_minor():
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 5


def test_new_entry_points_refuse_null_arguments():
    n, g = C.c_size_t(), C.c_size_t()
    L = N.lib
    assert L.fnnue_topk_children_device(None, None, None, None, None, None, 1, 1, None, None, 1, None) == E_ARG
    assert L.fnnue_topk_children(None, None, None, None, None, None, 1, 1, None, None, 1) == E_ARG
    assert L.fnnue_search1_lines_device(None, None, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                        C.byref(g), None) == E_ARG
    assert L.fnnue_search1_lines(None, b"x", 1, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                 C.byref(g)) == E_ARG
    assert L.fnnue_backend_lines_bound(None, 1, C.byref(n)) == E_ARG
    a, _keep = B._acquired([B.AcquireResponseBody("b", "x", "", multipv=3)])
    assert L.fnnue_backend_lines_bound(a, 1, None) == E_ARG
    off = np.zeros(2, dtype=np.uint32)
    rc = np.zeros(1, dtype=np.int32)
    assert L.fnnue_backend_go_lines(None, a, 1, None, 0, N.ptr(off), N.ptr(rc), None, 0, N.ptr(off), 0) == E_ARG
    buf = C.create_string_buffer(8)
    assert L.fnnue_backend_analysis_json_lines(None, 1, None, N.ptr(off), buf, 8, C.byref(n)) == E_ARG
    r = (B._Response * 1)()
    assert L.fnnue_backend_analysis_json_lines(r, 1, None, None, buf, 8, C.byref(n)) == E_ARG
    assert L.fnnue_backend_analysis_json_lines(r, 1, None, N.ptr(off), buf, 8, None) == E_ARG
    assert b"null" in L.fnnue_last_error()


@pytest.mark.parametrize("k", [0, 219, 2**32 - 1])
def test_search1_lines_refuses_other_k(k):
    n, g = C.c_size_t(), C.c_size_t()
    ctx = None  # the message says which check refused
    assert N.lib.fnnue_search1_lines_device(ctx, None, None, None, 1, k, None, 0, None, 0, None, 0, C.byref(n),
                                            C.byref(g), None) == E_ARG
    assert N.lib.fnnue_search1_lines(ctx, b"x", 1, None, None, 1, k, None, 0, None, 0, None, 0, C.byref(n),
                                     C.byref(g)) == E_ARG
    assert b"k must be" in N.lib.fnnue_last_error()


FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def test_lines_bound():
    body = lambda moves, **kw: B.AcquireResponseBody("b", FEN, moves, **kw)
    assert B.lines_bound([]) == 0
    assert B.lines_bound([body("e2e4 e7e5")]) == 0                                # multipv None
    assert B.lines_bound([body("e2e4 e7e5", work="move", multipv=3)]) == 0        # move work
    assert B.lines_bound([body("e2e4 e7e5 g1f3 b8c6", multipv=3)]) == 15          # (4 + 1) * 3
    assert B.lines_bound([body("", multipv=255)]) == 218                          # min(multipv, 218)
    assert B.lines_bound([body("e2e4", multipv=1)]) == 2
    assert B.lines_bound([body("e2e4 e7e5 g1f3 b8c6", multipv=3, skip_positions=[0, 1]),  # skips are not subtracted
                          body("e2e4"), body("", multipv=255), body("e2e4", multipv=1),
                          body("e2e4", work="move"), body("e2e4 e7e5", multipv=5, variant="crazyhouse")]) == \
        15 + 0 + 218 + 2 + 0 + 15


def resp(pid, kind, value, depth, nodes, move=None, matrix=True, time_ms=7, nps=0, lines=None):
    return B.PositionResponse(pid, B.Score(kind, value), 1, 2, depth, nodes, time_ms, nps, move, matrix=matrix,
                              lines=lines)


def line(kind, value, move):
    return B.PvLine(B.Score(kind, value), move, -3, 4)


def test_json_two_and_three_lines():
    assert B.into_analysis([resp(0, "cp", 31, 1, 20, "e2e4", lines=[line("cp", 31, "e2e4"), line("cp", 28, "d2d4")])]) \
        == '[{"pv":[[null,["e2e4"]],[null,["d2d4"]]],"score":[[null,{"cp":31}],[null,{"cp":28}]],' \
           '"depth":1,"nodes":20,"time":7}]'
    assert B.into_analysis([resp(4, "mate", 1, 1, 23, "f7g7", nps=900,
                                 lines=[line("mate", 1, "f7g7"), line("mate", 1, "f7f8"), line("cp", -12, "f6g6")])]) \
        == '[{"pv":[[null,["f7g7"]],[null,["f7f8"]],[null,["f6g6"]]],' \
           '"score":[[null,{"mate":1}],[null,{"mate":1}],[null,{"cp":-12}]],"depth":1,"nodes":23,"time":7,"nps":900}]'


def test_json_promotion_text():
    assert B.into_analysis([resp(0, "cp", 4, 1, 3, "a7a8q", lines=[line("cp", 4, "a7a8q"), line("cp", 1, "a7a8n")])]) \
        == '[{"pv":[[null,["a7a8q"]],[null,["a7a8n"]]],"score":[[null,{"cp":4}],[null,{"cp":1}]],' \
           '"depth":1,"nodes":3,"time":7}]'


def test_json_responses_without_lines_beside_one_with():
    got = B.into_analysis([
        resp(0, "cp", 31, 1, 20, "e2e4", lines=[line("cp", 31, "e2e4"), line("cp", 28, "d2d4")]),
        resp(1, "mate", 0, 0, 0),                                     # no legal move: no line
        B.PositionResponse(2, None, skipped=True),
        resp(3, "cp", 9, 1, 2, "a2a3", lines=[line("cp", 9, "a2a3")]),
        resp(4, "cp", -25, 1, 20, "e7e5", matrix=False)])
    assert got == \
        '[{"pv":[[null,["e2e4"]],[null,["d2d4"]]],"score":[[null,{"cp":31}],[null,{"cp":28}]],' \
        '"depth":1,"nodes":20,"time":7},' \
        '{"pv":[[[]]],"score":[[{"mate":0}]],"depth":0,"nodes":0,"time":7},' \
        '{"skipped":true},' \
        '{"pv":[[null,["a2a3"]]],"score":[[null,{"cp":9}]],"depth":1,"nodes":2,"time":7},' \
        '{"pv":"e7e5","score":{"cp":-25},"depth":1,"nodes":20,"time":7}]'


def as_c(responses):
    arr = (B._Response * max(1, len(responses)))()
    for i, r in enumerate(responses):
        if r.skipped:
            arr[i] = B._Response(r.position_id, 1)
            continue
        arr[i] = B._Response(r.position_id, 0, B.SCORE_MATE if r.score.kind == "mate" else B.SCORE_CP, r.depth,
                             1 if r.matrix else 0, r.score.value, r.psqt, r.positional, r.nodes, r.time_ms, r.nps,
                             (r.best_move or "").encode())
    return arr


def json_both(responses, with_line):
    """(fnnue_backend_analysis_json, fnnue_backend_analysis_json_lines) of the same responses, the second with
    each response's own line (where `with_line` says so) or none."""
    arr = as_c(responses)
    counts = [1 if with_line(r) else 0 for r in responses]
    loff = np.zeros(len(responses) + 1, dtype=np.uint32)
    loff[1:] = np.cumsum(counts)
    loff += 5  # relative to r[0]: any base
    pv = (B._PvLine * max(1, sum(counts)))()
    at = 0
    for r, c in zip(responses, counts):
        if c:
            pv[at] = B._PvLine(r.score.value, r.psqt, r.positional, (r.best_move or "").encode(),
                               B.SCORE_MATE if r.score.kind == "mate" else B.SCORE_CP)
            at += 1
    n = C.c_size_t()
    buf = C.create_string_buffer(4096)
    N.check(N.lib.fnnue_backend_analysis_json(arr, len(responses), buf, len(buf), C.byref(n)))
    old = buf.value.decode()
    N.check(N.lib.fnnue_backend_analysis_json_lines(arr, len(responses), pv, N.ptr(loff), buf, len(buf), C.byref(n)))
    return old, buf.value.decode()


# the responses of tests/test_search1.py's JSON tests
ONE_LINE_CASES = [
    [resp(0, "cp", 13, 0, 1, matrix=False)],
    [resp(0, "mate", 0, 0, 0, nps=5)],
    [B.PositionResponse(0, None, skipped=True)],
    [resp(0, "cp", -25, 1, 20, "e2e4", matrix=False, nps=1000)],
    [resp(3, "mate", 1, 1, 31, "d8h4", matrix=False)],
    [resp(0, "cp", 4, 1, 3, "a7a8q", matrix=False)],
    [resp(0, "cp", 31, 1, 20, "e2e4")],
    [resp(0, "mate", 1, 1, 2, "f7g7"), resp(1, "mate", 0, 0, 0), B.PositionResponse(2, None, skipped=True)],
]


@pytest.mark.parametrize("responses", ONE_LINE_CASES)
def test_json_equals_the_old_form_with_at_most_one_line(responses):
    has_move = lambda r: not r.skipped and r.best_move is not None
    for with_line in (lambda r: False, has_move):
        old, new = json_both(responses, with_line)
        assert new == old
    assert B.into_analysis(responses) == old


def test_json_capacity_protocol():
    responses = [resp(0, "cp", 31, 1, 20, "e2e4", lines=[line("cp", 31, "e2e4"), line("cp", 28, "d2d4")])]
    want = B.into_analysis(responses)
    arr = as_c(responses)
    pv = (B._PvLine * 2)(B._PvLine(31, 0, 0, b"e2e4", 0), B._PvLine(28, 0, 0, b"d2d4", 0))
    loff = np.array([0, 2], dtype=np.uint32)
    n = C.c_size_t()
    buf = C.create_string_buffer(len(want))  # one byte short of the text and its NUL
    assert N.lib.fnnue_backend_analysis_json_lines(arr, 1, pv, N.ptr(loff), buf, len(buf), C.byref(n)) == E_CAPACITY
    assert n.value == len(want)
    assert N.lib.fnnue_backend_analysis_json_lines(arr, 1, pv, N.ptr(loff), None, 0, C.byref(n)) == E_CAPACITY
    assert n.value == len(want)
    buf = C.create_string_buffer(len(want) + 1)
    assert N.lib.fnnue_backend_analysis_json_lines(arr, 1, pv, N.ptr(loff), buf, len(buf), C.byref(n)) == 0
    assert buf.value.decode() == want

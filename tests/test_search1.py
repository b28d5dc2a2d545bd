"""The host side of the one-ply search (ABI 3.4): move codes as UCI text, the
`analysis` JSON with a pv (AnalysisPart::Best, [ref] src/api.rs:359-369) and
the matrix form at depth 1 (Matrix::set, [ref] src/ipc.rs:77-86), the layout
of fnnue_best, and the no-device error paths of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B

E_ARG = -1


def sq(name: str) -> int:
    return (ord(name[1]) - ord("1")) * 8 + ord(name[0]) - ord("a")


def code(frm: str, to: str, promo: int = 0) -> int:
    return sq(frm) | sq(to) << 6 | promo << 12


def test_move_uci_on_hand_made_codes():
    assert F.move_uci(code("g1", "f3")) == "g1f3"
    assert [F.move_uci(code("e7", "e8", p)) for p in (2, 3, 4, 5)] == ["e7e8n", "e7e8b", "e7e8r", "e7e8q"]
    assert F.move_uci(code("a2", "b1", 5)) == "a2b1q"
    assert F.move_uci(code("e1", "g1")) == "e1g1"      # castling as the game's notation spells it
    assert F.move_uci(code("g1", "h1")) == "g1h1"      # Chess960: the king takes its rook
    assert F.move_uci(code("a1", "h8")) == "a1h8"
    assert F.move_uci(0) == ""                         # no move


@pytest.mark.parametrize("promo", [1, 6, 7])
def test_move_uci_refuses_other_promotions(promo):
    buf = C.create_string_buffer(8)
    assert N.lib.fnnue_move_uci(code("e7", "e8", promo), buf) == E_ARG
    with pytest.raises(F.FnnueError) as e:
        F.move_uci(code("e7", "e8", promo))
    assert e.value.code == E_ARG


def test_move_uci_null_and_high_bit():
    assert N.lib.fnnue_move_uci(code("e2", "e4"), None) == E_ARG
    assert N.lib.fnnue_move_uci(code("e2", "e4") | 0x8000, C.create_string_buffer(8)) == E_ARG


def test_best_record_layout():
    assert C.sizeof(F.Best) == 24 and N.BEST_BYTES == 24 and F.BEST_DTYPE.itemsize == 24
    assert [(n, F.BEST_DTYPE.fields[n][1]) for n in F.BEST_DTYPE.names] == \
        [(n, getattr(F.Best, n).offset) for n, _ in F.Best._fields_]
    assert (F.Best.move.offset, F.Best.kind.offset, F.Best.end.offset) == (20, 22, 23)
    assert (F.BEST_NONE, F.BEST_CP, F.BEST_MATE) == (0, 1, 2)


def test_abi_minor():
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 4


def resp(pid, kind, value, depth, nodes, move=None, matrix=False, time_ms=7, nps=0):
    return B.PositionResponse(pid, B.Score(kind, value), 1, 2, depth, nodes, time_ms, nps, move, matrix=matrix)


def test_json_depth0_forms_unchanged():
    assert B.into_analysis([resp(0, "cp", 13, 0, 1)]) == '[{"score":{"cp":13},"depth":0,"nodes":1,"time":7}]'
    assert B.into_analysis([resp(0, "mate", 0, 0, 0, matrix=True, nps=5)]) == \
        '[{"pv":[[[]]],"score":[[{"mate":0}]],"depth":0,"nodes":0,"time":7,"nps":5}]'
    assert B.into_analysis([B.PositionResponse(0, None, skipped=True)]) == '[{"skipped":true}]'


def test_json_best_with_pv():
    assert B.into_analysis([resp(0, "cp", -25, 1, 20, "e2e4", nps=1000)]) == \
        '[{"pv":"e2e4","score":{"cp":-25},"depth":1,"nodes":20,"time":7,"nps":1000}]'
    assert B.into_analysis([resp(3, "mate", 1, 1, 31, "d8h4")]) == \
        '[{"pv":"d8h4","score":{"mate":1},"depth":1,"nodes":31,"time":7}]'
    assert B.into_analysis([resp(0, "cp", 4, 1, 3, "a7a8q")]) == \
        '[{"pv":"a7a8q","score":{"cp":4},"depth":1,"nodes":3,"time":7}]'


def test_json_matrix_at_depth1():
    assert B.into_analysis([resp(0, "cp", 31, 1, 20, "e2e4", matrix=True)]) == \
        '[{"pv":[[null,["e2e4"]]],"score":[[null,{"cp":31}]],"depth":1,"nodes":20,"time":7}]'
    assert B.into_analysis([resp(0, "mate", 1, 1, 2, "f7g7", matrix=True),
                            resp(1, "mate", 0, 0, 0, matrix=True),
                            B.PositionResponse(2, None, skipped=True)]) == \
        '[{"pv":[[null,["f7g7"]]],"score":[[null,{"mate":1}]],"depth":1,"nodes":2,"time":7},' \
        '{"pv":[[[]]],"score":[[{"mate":0}]],"depth":0,"nodes":0,"time":7},{"skipped":true}]'


def test_new_entry_points_refuse_null_arguments():
    n, g = C.c_size_t(), C.c_size_t()
    L = N.lib
    assert L.fnnue_build_children_device(None, None, None, None, 1, None, 0, None, 0, None, None, C.byref(n),
                                         C.byref(g), None) == E_ARG
    assert L.fnnue_build_children(None, b"x", 1, None, None, 1, None, 0, None, 0, None, None, C.byref(n),
                                  C.byref(g)) == E_ARG
    assert L.fnnue_best_children_device(None, None, None, None, None, None, 1, 1, None, None) == E_ARG
    assert L.fnnue_best_children(None, None, None, None, None, None, 1, 1, None) == E_ARG
    assert L.fnnue_search1_device(None, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g), None) == E_ARG
    assert L.fnnue_search1(None, b"x", 1, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert b"null" in L.fnnue_last_error()


def test_set_analysis_depth_null_backend():
    assert N.lib.fnnue_backend_set_analysis_depth(None, 1) == E_ARG
    assert N.lib.fnnue_backend_set_analysis_depth(None, 0) == E_ARG

"""The host side of the variant one-ply search (ABI 3.6): variant move codes
as UCI text (drops "N@f3"), the ABI version, the new constants and the
no-device error paths of the new entry points and of the variant depth
setter."""
import ctypes as C

import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B

E_ARG = -1


def sq(name: str) -> int:
    return (ord(name[1]) - ord("1")) * 8 + ord(name[0]) - ord("a")


def code(frm: str, to: str, promo: int = 0) -> int:
    return sq(frm) | sq(to) << 6 | promo << 12


def drop(piece: str, to: str) -> int:
    return code(to, to, " PNBRQ".index(piece))


def test_vmove_uci_known_answers():
    assert F.vmove_uci(code("e2", "e4")) == "e2e4"
    assert F.vmove_uci(code("e7", "e8", 5)) == "e7e8q"
    assert [F.vmove_uci(code("a7", "b8", p)) for p in (2, 3, 4, 5)] == ["a7b8n", "a7b8b", "a7b8r", "a7b8q"]
    assert F.vmove_uci(drop("P", "e4")) == "P@e4"
    assert F.vmove_uci(drop("Q", "h8")) == "Q@h8"
    assert F.vmove_uci(drop("N", "f3")) == "N@f3"
    assert [F.vmove_uci(drop(p, "a1")) for p in "PNBRQ"] == ["P@a1", "N@a1", "B@a1", "R@a1", "Q@a1"]
    assert F.vmove_uci(code("e1", "g1")) == "e1g1"  # castling as the game's notation spells it
    assert F.vmove_uci(code("e1", "h1")) == "e1h1"  # Chess960: the king takes its rook
    assert F.vmove_uci(0) == ""                     # no move


def test_vmove_uci_equals_move_uci_on_ordinary_moves():
    for m in (code("g1", "f3"), code("a2", "b1", 5), code("a1", "h8"), code("h7", "h8", 2), 0):
        assert F.vmove_uci(m) == F.move_uci(m)


REFUSED = [
    code("e4", "e4", 0),          # from == to without a piece (the code 0 itself, a1a1, is "no move")
    code("h8", "h8", 0),
    code("e4", "e4", 6), code("e4", "e4", 7),
    code("e7", "e8", 6), code("e7", "e8", 7),
    code("e7", "e8", 1),          # a promotion to a pawn, as fnnue_move_uci refuses it
    code("e2", "e4") | 0x8000,    # bit 15
    drop("N", "f3") | 0x8000,
    0x8000,
]


@pytest.mark.parametrize("m", REFUSED)
def test_vmove_uci_refuses(m):
    buf = C.create_string_buffer(b"zzzzzzz", 8)
    assert N.lib.fnnue_vmove_uci(m, buf) == E_ARG
    assert buf.value == b""
    with pytest.raises(F.FnnueError) as e:
        F.vmove_uci(m)
    assert e.value.code == E_ARG


def test_vmove_uci_null_out():
    assert N.lib.fnnue_vmove_uci(code("e2", "e4"), None) == E_ARG
    assert N.lib.fnnue_vmove_uci(drop("N", "f3"), None) == E_ARG
    assert N.lib.fnnue_vmove_uci(0, None) == E_ARG


def test_move_uci_still_refuses_drops_and_pawn_promotions():
    buf = C.create_string_buffer(8)
    assert N.lib.fnnue_move_uci(drop("P", "e4"), buf) == E_ARG          # promo 1
    assert N.lib.fnnue_move_uci(code("e7", "e8", 1), buf) == E_ARG


def test_abi_minor_and_constants():
    assert N.lib.fnnue_abi_version() >= (3 << 16) | 6
    assert N.lib.fnnue_abi_version() >> 16 == 3
    assert F.END_WON == 0x40 and F.BEST_LOST == 3
    assert (F.BEST_NONE, F.BEST_CP, F.BEST_MATE) == (0, 1, 2)


def test_new_entry_points_refuse_null_arguments():
    n, g = C.c_size_t(), C.c_size_t()
    L = N.lib
    V = N.VARIANT_CRAZYHOUSE
    assert L.fnnue_build_vchildren_device(None, V, None, None, None, 1, None, 0, None, 0, None, None, C.byref(n),
                                          C.byref(g), None) == E_ARG
    assert L.fnnue_build_vchildren(None, V, b"x", 1, None, None, 1, None, 0, None, 0, None, None, C.byref(n),
                                   C.byref(g)) == E_ARG
    assert L.fnnue_vsearch1_device(None, V, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g),
                                   None) == E_ARG
    assert L.fnnue_vsearch1(None, V, b"x", 1, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(g)) == E_ARG
    assert L.fnnue_vsearch1_lines_device(None, V, None, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                         C.byref(g), None) == E_ARG
    assert L.fnnue_vsearch1_lines(None, V, b"x", 1, None, None, 1, 3, None, 0, None, 0, None, 0, C.byref(n),
                                  C.byref(g)) == E_ARG
    assert b"null" in L.fnnue_last_error()
    # the counts too
    assert L.fnnue_vsearch1(None, V, b"x", 1, None, None, 1, None, 0, None, 0, None, None) == E_ARG
    assert L.fnnue_build_vchildren(None, V, b"x", 1, None, None, 1, None, 0, None, 0, None, None, None, None) == E_ARG


@pytest.mark.parametrize("k", [0, N.MAX_CHILDREN + 1])
def test_vsearch1_lines_refuses_k(k):
    n, g = C.c_size_t(), C.c_size_t()
    assert N.lib.fnnue_vsearch1_lines(None, N.VARIANT_ATOMIC, b"x", 1, None, None, 1, k, None, 0, None, 0, None, 0,
                                      C.byref(n), C.byref(g)) == E_ARG


def test_set_variant_analysis_depth_null_backend():
    assert N.lib.fnnue_backend_set_variant_analysis_depth(None, 1) == E_ARG
    assert N.lib.fnnue_backend_set_variant_analysis_depth(None, 0) == E_ARG
    assert N.lib.fnnue_backend_set_variant_analysis_depth(None, 2) == E_ARG


def test_json_carries_a_drop_as_pv():
    r = B.PositionResponse(0, B.Score("cp", 12), 1, 2, 1, 64, 7, 0, "N@f3")
    assert B.into_analysis([r]) == '[{"pv":"N@f3","score":{"cp":12},"depth":1,"nodes":64,"time":7}]'
    r = B.PositionResponse(0, B.Score("mate", -1), 1, 2, 1, 3, 7, 0, "e7e8")
    assert B.into_analysis([r]) == '[{"pv":"e7e8","score":{"mate":-1},"depth":1,"nodes":3,"time":7}]'

"""No-GPU checks of the boundary of the game records: omok_game_log_enable, omok_game_log_read and omok_env_replay exist in
include/omok_mi355x.h, in bindings/omok_mi355x.rs and in the library, with matching signatures, and the ctypes mirror declares them."""
import ctypes as C
import importlib.util
import os

from omok_ai_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I32, ENGINE = ("int", 32, ()), ("engine", 0, ("mut",))
U8_IN, U8_OUT, I32_IN, I32_OUT = ("uint", 8, ("const",)), ("uint", 8, ("mut",)), ("int", 32, ("const",)), ("int", 32, ("mut",))
U32_OUT, F32_OUT = ("uint", 32, ("mut",)), ("float", 32, ("mut",))
WANT = {
    "omok_game_log_enable": [("e", ENGINE), ("enabled", I32)],
    "omok_game_log_read": [("e", ENGINE), ("first_game", I32), ("games", I32), ("start_boards", U8_OUT), ("lengths", I32_OUT),
                           ("moves", ("uint", 16, ("mut",))), ("root_n", U32_OUT), ("root_w", F32_OUT), ("child_n", U32_OUT), ("child_w", F32_OUT)],
    "omok_env_replay": [("e", ENGINE), ("start_boards", U8_IN), ("moves", ("uint", 16, ("const",))), ("lengths", I32_IN), ("batch", I32),
                        ("stride", I32), ("upto", I32), ("boards_out", U8_OUT), ("status_out", I32_OUT), ("played_out", I32_OUT)],
}
CTYPES = {
    "omok_game_log_enable": [C.c_void_p, C.c_int32],
    "omok_game_log_read": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint16),
                           C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)],
    "omok_env_replay": [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                        C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
}


def _abi_text():
    spec = importlib.util.spec_from_file_location("abi_text", os.path.join(ROOT, "tools", "abi_text.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_the_three_entry_points():
    c = _abi_text().parse_header()
    for name, args in WANT.items():
        assert name in c, name
        ret, got = c[name]
        assert ret == ("cint", 32, ()), (name, ret)
        assert got == args, (name, got)


def test_header_and_rust_text_agree_on_the_move_word():
    A = _abi_text()
    c, rs = A.parse_defines(), A.parse_rust_consts()
    assert c["OMOK_MOVE_CELL"] == rs["OMOK_MOVE_CELL"] == 0xFF
    assert c["OMOK_MOVE_EXTERNAL"] == rs["OMOK_MOVE_EXTERNAL"] == 0x100


def test_rust_binding_declares_them_like_the_header():
    A = _abi_text()
    c, rs = A.parse_header(), A.parse_rust()
    for name in WANT:
        assert name in rs, name
        assert rs[name][0] == c[name][0], (name, "return")
        assert [t for _, t in rs[name][1]] == [t for _, t in c[name][1]], (name, "arguments")


def test_library_and_ctypes_mirror_have_them():
    assert os.path.exists(binding.LIB_PATH), "run __graft_entry__.build() first"
    raw = C.CDLL(binding.LIB_PATH)
    lib = binding.lib()
    for name, args in CTYPES.items():
        assert name in binding.SYMBOLS, name
        assert hasattr(raw, name), name
        assert list(getattr(lib, name).argtypes) == args, name

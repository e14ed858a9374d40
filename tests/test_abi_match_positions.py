"""No-GPU checks of the boundary of the matches from given positions: omok_match_reset_from and omok_env_random_positions exist in
include/omok_mi355x.h, in bindings/omok_mi355x.rs and in the library, with matching signatures, and the ctypes mirror declares them."""
import ctypes as C
import importlib.util
import os

from omok_ai_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I32, ENGINE = ("int", 32, ()), ("engine", 0, ("mut",))
WANT = {
    "omok_match_reset_from": [("e", ENGINE), ("split", I32), ("boards", ("uint", 8, ("const",)))],
    "omok_env_random_positions": [("e", ENGINE), ("key", ("uint", 64, ())), ("first_game", ("int", 64, ())), ("stones", I32), ("batch", I32),
                                  ("boards_out", ("uint", 8, ("mut",))), ("ok_out", ("uint", 8, ("mut",)))],
}


def _abi_text():
    spec = importlib.util.spec_from_file_location("abi_text", os.path.join(ROOT, "tools", "abi_text.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_the_two_entry_points():
    c = _abi_text().parse_header()
    for name, args in WANT.items():
        assert name in c, name
        ret, got = c[name]
        assert ret == ("cint", 32, ()), (name, ret)
        assert got == args, (name, got)


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
    for name, args in WANT.items():
        assert name in binding.SYMBOLS, name
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == len(args), name

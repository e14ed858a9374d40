"""No-GPU checks of the slots-mode move log: records.GameRecords.from_packed on hand-made entries (the 20-byte layout of
omok_selfplay_run_slots_logged: root_n u32, root_w f32, child_n u32, child_w f32, move u16, zero u16, little-endian), and the presence of
omok_game_log_entry_bytes and omok_selfplay_run_slots_logged in the header, the generated Rust binding, the ctypes mirror and the library."""
import ctypes as C
import importlib.util
import os
import struct

import numpy as np
import pytest

from omok_ai_amd import binding, records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HW = 3, 9
NEG_ZERO, NAN_PAYLOAD = 0x80000000, 0x7FC12345  # root_w of two entries, as their words


def _entry(root_n, root_w_bits, child_n, child_w_bits, move, pad=0):
    return struct.pack("<IIIIHH", root_n, root_w_bits, child_n, child_w_bits, move, pad)


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _games():
    """three games by index: 0 = 2 moves (one external), 1 = no move, 2 = HW moves; (root_n, root_w bits, child_n, child_w bits, move) each"""
    g0 = [(16, NEG_ZERO, 5, _f32_bits(1.5), 4), (24, NAN_PAYLOAD, 0, 0, 7 | 0x100)]
    g2 = [(100 + i, _f32_bits(-0.25 * i), 10 + i, _f32_bits(0.5 * i), (i * 2) % HW) for i in range(HW)]
    return [g0, [], g2]


def _packed(pad_at=None):
    """game 2 first at entry 1, a gap, game 0 at entry 12, game 1 (length 0) pointing at the end; unused entries hold 0xEE bytes"""
    games = _games()
    offsets, lengths = np.array([12, 14, 1], dtype=np.int64), np.array([2, 0, HW], dtype=np.int32)
    buf = np.full((14, R.ENTRY_BYTES), 0xEE, dtype=np.uint8)
    for g, entries in enumerate(games):
        for i, e in enumerate(entries):
            pad = 1 if pad_at == (g, i) else 0
            buf[offsets[g] + i] = np.frombuffer(_entry(*e, pad), dtype=np.uint8)
    return buf, offsets, lengths, np.array([2, 0, 1], dtype=np.int32)


def _by_hand():
    """the padded arrays of omok_game_log_read for the same games, written out field by field"""
    games = _games()
    moves = np.full((3, HW), 0xFFFF, dtype=np.uint16)
    root_n, root_w, child_n, child_w = (np.zeros((3, HW), dtype=np.uint32) for _ in range(4))
    for g, entries in enumerate(games):
        for i, (rn, rw, cn, cw, mv) in enumerate(entries):
            root_n[g, i], root_w[g, i], child_n[g, i], child_w[g, i], moves[g, i] = rn, rw, cn, cw, mv
    return moves, root_n, root_w, child_n, child_w


def test_from_packed_returns_the_padded_arrays():
    buf, offsets, lengths, status = _packed()
    rec = R.GameRecords.from_packed(N, buf, offsets, lengths, status, meta={"kind": "selfplay"})
    moves, root_n, root_w, child_n, child_w = _by_hand()
    assert rec.n == N and rec.games == 3 and rec.meta == {"kind": "selfplay"}
    assert rec.moves().dtype == np.uint16 and np.array_equal(rec.moves(), moves)
    assert np.array_equal(rec.lengths, [2, 0, HW]) and np.array_equal(rec.plies, [2, 0, HW]) and rec.plies.dtype == np.int32
    assert rec.status.dtype == np.uint8 and np.array_equal(rec.status, [2, 0, 1])
    assert not rec.start_boards.any() and rec.start_boards.shape == (3, HW)
    assert rec.root_n.dtype == np.uint32 and np.array_equal(rec.root_n, root_n)
    assert rec.child_n.dtype == np.uint32 and np.array_equal(rec.child_n, child_n)
    assert rec.root_w.dtype == np.float32 and np.array_equal(rec.root_w.view(np.uint32), root_w)  # -0.0 and the NaN's payload survive
    assert rec.child_w.dtype == np.float32 and np.array_equal(rec.child_w.view(np.uint32), child_w)
    assert rec.root_w.view(np.uint32)[0, 0] == NEG_ZERO and rec.root_w.view(np.uint32)[0, 1] == NAN_PAYLOAD
    assert rec.cells[0, 0] == 4 and rec.cells[0, 1] == 7 and (rec.cells[0, 2:] == -1).all() and (rec.cells[1] == -1).all()
    assert rec.external[0, 1] and rec.external.sum() == 1


def test_from_packed_equals_from_log_and_survives_a_file(tmp_path):
    buf, offsets, lengths, status = _packed()
    rec = R.GameRecords.from_packed(N, buf, offsets, lengths, status, meta={"iteration": 3})
    moves, root_n, root_w, child_n, child_w = _by_hand()
    want = R.GameRecords.from_log(N, np.zeros((3, HW), np.uint8), lengths, moves, root_n, root_w.view(np.float32), child_n, child_w.view(np.float32),
                                  status.astype(np.uint8), lengths, meta={"iteration": 3})
    assert rec == want
    path = str(tmp_path / "games.npz")
    rec.save(path)
    assert R.load(path) == rec
    assert R.load(path).root_w.view(np.uint32)[0, 1] == NAN_PAYLOAD
    assert R.main(["show", path, "--game", "2"]) == 0


def test_from_packed_of_no_games_and_no_entries():
    rec = R.GameRecords.from_packed(N, np.zeros((0, R.ENTRY_BYTES), np.uint8), [], [], [])
    assert rec.games == 0 and rec.cells.shape == (0, HW)
    rec = R.GameRecords.from_packed(N, np.zeros((0, R.ENTRY_BYTES), np.uint8), [0], [0], [0])
    assert rec.games == 1 and (rec.cells == -1).all()


def test_from_packed_rejects_inconsistent_fields():
    buf, offsets, lengths, status = _packed()
    with pytest.raises(ValueError):  # game 0 reaches one entry beyond the buffer
        R.GameRecords.from_packed(N, buf, np.array([13, 14, 1]), lengths, status)
    with pytest.raises(ValueError):  # a negative offset
        R.GameRecords.from_packed(N, buf, np.array([-1, 14, 1]), lengths, status)
    with pytest.raises(ValueError):  # a length beyond HW
        R.GameRecords.from_packed(N, buf, np.array([0, 14, 1]), np.array([HW + 1, 0, HW]), status)
    with pytest.raises(ValueError):  # a negative length
        R.GameRecords.from_packed(N, buf, offsets, np.array([2, -1, HW]), status)
    with pytest.raises(ValueError):  # a non-zero pad in a played entry
        R.GameRecords.from_packed(N, _packed(pad_at=(2, HW - 1))[0], offsets, lengths, status)
    with pytest.raises(ValueError):  # entries of another width
        R.GameRecords.from_packed(N, buf[:, :19], offsets, lengths, status)
    with pytest.raises(ValueError):  # arrays of different game counts
        R.GameRecords.from_packed(N, buf, offsets, lengths, status[:2])


# ---- the boundary ---------------------------------------------------------------------------------
I32, I64, F32, ENGINE = ("int", 32, ()), ("int", 64, ()), ("float", 32, ()), ("engine", 0, ("mut",))
VOID_MUT, I64_OUT, I32_OUT, F64_OUT = ("void", 0, ("mut",)), ("int", 64, ("mut",)), ("int", 32, ("mut",)), ("float", 64, ("mut",))
NEW = ("omok_game_log_entry_bytes", "omok_selfplay_run_slots_logged")


def _abi_text():
    spec = importlib.util.spec_from_file_location("abi_text", os.path.join(ROOT, "tools", "abi_text.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_the_logged_run_as_run_slots_plus_the_log_buffer():
    c = _abi_text().parse_header()
    for name in NEW:
        assert name in c, name
    assert c["omok_game_log_entry_bytes"] == (("int", 32, ()), [])
    ret, args = c["omok_selfplay_run_slots_logged"]
    plain_ret, plain = c["omok_selfplay_run_slots"]
    assert ret == plain_ret
    at = [name for name, _ in plain].index("cap_records") + 1
    assert args[:at] == plain[:at] and args[at + 1:] == plain[at:]
    assert args[at][0] == "log_dev" and args[at][1] == dict(plain)["records_dev"]


def test_rust_binding_declares_them_like_the_header():
    A = _abi_text()
    c, rs = A.parse_header(), A.parse_rust()
    for name in NEW:
        assert name in rs, name
        assert rs[name][0] == c[name][0], (name, "return")
        assert [t for _, t in rs[name][1]] == [t for _, t in c[name][1]], (name, "arguments")


def test_library_and_ctypes_mirror_have_them():
    assert os.path.exists(binding.LIB_PATH), "run __graft_entry__.build() first"
    raw = C.CDLL(binding.LIB_PATH)
    lib = binding.lib()
    for name in NEW:
        assert name in binding.SYMBOLS, name
        assert hasattr(raw, name), name
    assert lib.omok_game_log_entry_bytes() == R.ENTRY_BYTES == 20  # (needs no engine and no GPU)
    plain = list(lib.omok_selfplay_run_slots.argtypes)
    assert list(lib.omok_selfplay_run_slots_logged.argtypes) == plain[:10] + [C.c_void_p] + plain[10:]

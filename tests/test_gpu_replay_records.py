"""omok_replay_augment_records_dev: the replay post-processing of Trainer::train (src/trainer.rs:207-324: z back-fill, five augmented copies per
transition, src/utils.rs:1-64) on caller-held packed records -- what slots mode hands back -- must write, byte for byte, what
omok_replay_augment_dev writes for an engine that holds the same games in the same index order.  Yardsticks: the engine's own
replay_augment_into and oracle.replay_postprocess (pinned by tests/test_replay_postprocess.py); for the synthetic extremes a numpy statement of
the five transforms."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import omok_ai_amd as oa  # noqa: E402
from omok_ai_amd import binding as B  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_INVALID = -1  # OMOK_ERR_INVALID (include/omok_mi355x.h)
FILL = 0xCC


def _layout(n):
    hw = n * n
    brd = (hw + 1 + 3) // 4 * 4
    return hw, brd, brd + 4 * hw + 4


def _call(eng, src, offs, lens, cap=None, slack=3):
    """the new call on the host array src [records][REC]; (returned count, dst [cap + slack][REC] as left on the device, FILL where unwritten)"""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    rec = src.shape[1]
    total = 6 * int(np.maximum(np.asarray(lens, dtype=np.int64), 0).sum())
    cap = total if cap is None else cap
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full(((max(total, cap) + slack) * rec,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = eng.replay_augment_records(d_src.data_ptr(), src.shape[0], offs, lens, d_dst.data_ptr(), cap)
    return got, d_dst.cpu().numpy().reshape(-1, rec)


# ---- 1, 2, 5: one short whole episode per board size, shared by the tests below (nothing here is changed after it is made) ----
_EPISODES = {}


def _episode(n):
    if n not in _EPISODES:
        games = 6
        eng = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=256, max_batch_k=8, seed=11)
        eng.load_random_weights(0)
        sp = oa.SelfPlay(eng)
        sp.reset()
        sp.run(16, 8, 0.25, 0.03, 1.0, 30, 0)
        rec = sp.replay_record_bytes()
        replays = [sp.replay(g) for g in range(games)]
        lens = np.array([len(r[1]) for r in replays], dtype=np.int32)
        raw_n = int(lens.sum())
        raw = torch.zeros(raw_n * rec, dtype=torch.uint8, device="cuda")
        assert sp.replay_pack_into(raw.data_ptr(), raw_n) == raw_n
        want = torch.zeros(6 * raw_n * rec, dtype=torch.uint8, device="cuda")
        assert sp.replay_augment_into(want.data_ptr(), 6 * raw_n) == 6 * raw_n
        _EPISODES[n] = {"eng": eng, "rec": rec, "replays": replays, "lens": lens, "offs": np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64),
                        "raw": raw.cpu().numpy().reshape(-1, rec), "want": want.cpu().numpy().reshape(-1, rec)}
    return _EPISODES[n]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for ep in _EPISODES.values():
        ep["eng"].close()
    _EPISODES.clear()


@pytest.mark.parametrize("n", [9, 15])
def test_same_bytes_as_the_engines_own_postprocessing(n):
    ep = _episode(n)
    hw, brd, rec = _layout(n)
    assert rec == ep["rec"] and (ep["lens"] > 0).all()
    got, dst = _call(ep["eng"], ep["raw"], ep["offs"], ep["lens"])
    assert got == 6 * int(ep["lens"].sum()) == len(ep["want"])
    assert np.array_equal(dst[:got], ep["want"])
    assert (dst[got:] == FILL).all()
    base = 0
    for g, (boards, turns, pi, z) in enumerate(ep["replays"]):  # ... and every game's block is the reference's post-processing of its raw transitions
        bo, to, po, zo = O.replay_postprocess(n, boards, turns, pi, z)
        blk = dst[base:base + len(to)]
        assert np.array_equal(blk[:, :hw], bo) and np.array_equal(blk[:, hw], to) and not blk[:, hw + 1:brd].any(), g
        assert np.array_equal(blk[:, brd:brd + 4 * hw].copy().view(np.uint32), po.view(np.uint32)), g
        assert np.array_equal(blk[:, brd + 4 * hw:].copy().view(np.uint32).ravel(), zo.view(np.uint32)), g
        base += len(to)
    assert base == got


@pytest.mark.parametrize("n", [9, 15])
def test_placement_of_the_games_in_the_source_buffer_does_not_matter(n):
    ep = _episode(n)
    rec, lens, games = ep["rec"], ep["lens"], len(ep["lens"])
    rng = np.random.default_rng(5 + n)
    order = rng.permutation(games)
    gaps = rng.integers(1, 8, games + 1)
    src = np.full((int(lens.sum()) + int(gaps.sum()), rec), 0xA5, dtype=np.uint8)
    offs = np.zeros(games, dtype=np.int64)
    at = int(gaps[0])
    for i, g in enumerate(order):  # games in shuffled order, 0xA5-filled gaps in front of, between and behind them
        offs[g] = at
        src[at:at + lens[g]] = ep["raw"][ep["offs"][g]:ep["offs"][g] + lens[g]]
        at += int(lens[g]) + int(gaps[i + 1])
    assert at == len(src) and not np.array_equal(order, np.arange(games))
    got, dst = _call(ep["eng"], src, offs, lens)
    assert got == len(ep["want"]) and np.array_equal(dst[:got], ep["want"]) and (dst[got:] == FILL).all()
    # a game of length 0 in the middle of the list (its offset points at a gap, even outside the buffer: never read) shifts nothing
    for empty_off in (0, len(src) + 99):
        offs0 = np.concatenate([offs[:3], [empty_off], offs[3:]])
        lens0 = np.concatenate([lens[:3], [0], lens[3:]]).astype(np.int32)
        got, dst = _call(ep["eng"], src, offs0, lens0)
        assert got == len(ep["want"]) and np.array_equal(dst[:got], ep["want"]) and (dst[got:] == FILL).all()


@pytest.mark.parametrize("n", [9, 15])
def test_truncation_returns_the_total_and_writes_the_first_cap_records_only(n):
    ep = _episode(n)
    total = len(ep["want"])
    cap = total - 9
    got, dst = _call(ep["eng"], ep["raw"], ep["offs"], ep["lens"], cap=cap)
    assert got == total
    assert np.array_equal(dst[:cap], ep["want"][:cap])
    assert (dst[cap:] == FILL).all()  # the bytes behind the capacity are untouched


# ---- 3: slots mode end to end (the parameters of tests/test_gpu_slots.py) ----
@pytest.mark.parametrize("n,slots,total,sims,k,mode", [
    (9, 6, 20, 32, 8, B.NET_F16X3),
    (15, 4, 10, 32, 16, B.NET_F16X3_ROWS),
])
def test_slots_mode_plus_the_new_call_equals_the_episodes_postprocessing(n, slots, total, sims, k, mode):
    seed, threshold, max_nodes = 21, 6, 1024
    _, _, rec = _layout(n)

    def engine(games):
        eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_nodes // 2, max_batch_k=k, seed=seed, net_mode=mode)
        eng.load_random_weights(0)
        sp = oa.SelfPlay(eng)
        sp.reset()
        return eng, sp

    eng, sp = engine(total)
    sp.run(sims, k, 0.25, 0.03, 1.0, threshold)
    _, _, plies = sp.game_info()
    want_n = 6 * int(plies.sum())
    want = torch.zeros(want_n * rec, dtype=torch.uint8, device="cuda")
    assert sp.replay_augment_into(want.data_ptr(), want_n) == want_n
    want = want.cpu().numpy()
    eng.close()

    eng, sp = engine(slots)
    cap = total * n * n
    raw = torch.zeros(cap * rec, dtype=torch.uint8, device="cuda")
    _, nrec, off, ln, _ = sp.run_slots(total, sims, k, raw.data_ptr(), cap, 0.25, 0.03, 1.0, threshold)
    dst = torch.full(((want_n + 2) * rec,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = eng.replay_augment_records(raw.data_ptr(), nrec, off, ln, dst.data_ptr(), want_n + 2)
    assert got == want_n == 6 * nrec
    dst = dst.cpu().numpy()
    assert np.array_equal(dst[:want_n * rec], want)
    assert (dst[want_n * rec:] == FILL).all()
    eng.close()


# ---- 4: synthetic extremes: no net, no search -- an engine is created and nothing is loaded ----
def _transform_maps(n):
    """src cell of every destination cell for rotate_90, rotate_180, rotate_270, flip_horizontal, flip_vertical (src/utils.rs:1-64), stated with
    numpy's own rotations and flips as tests/test_replay_postprocess.py states them"""
    idx = np.arange(n * n).reshape(n, n)
    return [f(idx).ravel() for f in (lambda a: np.rot90(a, -1), lambda a: np.rot90(a, 2), lambda a: np.rot90(a, 1), lambda a: a[:, ::-1], lambda a: a[::-1, :])]


def _synthetic(n, games, length, z_last, seed):
    """(records [games * length][REC] of random boards, turns and pi, games back to back in index order; the expected output [games * 6 * length][REC])"""
    hw, brd, rec = _layout(n)
    rng = np.random.default_rng(seed)
    t = games * length
    boards = rng.integers(0, 3, (t, hw), dtype=np.uint8)
    turns = rng.integers(0, 2, t, dtype=np.uint8)
    pi = rng.random((t, hw), dtype=np.float32)
    z = rng.choice(np.array([1.0, -1.0, 0.0, -0.0], np.float32), t).astype(np.float32)  # z as recorded at play time: all but a game's last are overwritten
    z.reshape(games, length)[:, -1] = z_last
    src = np.zeros((t, rec), dtype=np.uint8)
    src[:, :hw], src[:, hw] = boards, turns
    src[:, brd:brd + 4 * hw] = pi.view(np.uint8)
    src[:, brd + 4 * hw:] = z.view(np.uint8).reshape(t, 4)
    # expected: per game the L transitions with z back-filled, then [L][5] transformed copies
    zl = z.reshape(games, length)[:, -1:]
    odd = ((length - 1 - np.arange(length)) & 1).astype(bool)[None, :]
    zb = np.where(odd, -zl, zl).astype(np.float32).reshape(t)
    first = src.copy()
    first[:, brd + 4 * hw:] = zb.view(np.uint8).reshape(t, 4)
    copies = np.repeat(first[:, None, :], 5, axis=1)  # turn, pad and z as in the back-filled transition
    for k, m in enumerate(_transform_maps(n)):
        copies[:, k, :hw] = boards[:, m]
        copies[:, k, brd:brd + 4 * hw] = np.ascontiguousarray(pi[:, m]).view(np.uint8)
    want = np.concatenate([first.reshape(games, length, rec), copies.reshape(games, 5 * length, rec)], axis=1).reshape(6 * t, rec)
    return src, want


def test_seventy_thousand_games_of_one_transition():
    """more games than gridDim.y allows (65 535): the launch shape of omok_replay_augment_dev cannot be what runs here"""
    n, games = 9, 70_000
    eng = oa.Engine(board_size=n, games=1, max_nodes=64, max_tables=32, max_batch_k=8)
    rng = np.random.default_rng(3)
    z_last = rng.choice(np.array([1.0, -1.0, 0.0, -0.0], np.float32), games).astype(np.float32)
    src, want = _synthetic(n, games, 1, z_last, seed=4)
    got, dst = _call(eng, src, np.arange(games, dtype=np.int64), np.ones(games, np.int32))
    assert got == 6 * games
    assert np.array_equal(dst[:got], want)
    assert (dst[got:] == FILL).all()
    eng.close()


@pytest.mark.parametrize("n", [9, 15])
@pytest.mark.parametrize("z_last", [-0.0, 1.0])
def test_one_game_of_full_length_alternates_the_sign_bit_exactly(n, z_last):
    hw, brd, rec = _layout(n)
    eng = oa.Engine(board_size=n, games=1, max_nodes=64, max_tables=32, max_batch_k=8)
    src, want = _synthetic(n, 1, hw, np.float32(z_last), seed=n)
    got, dst = _call(eng, src, [0], [hw])
    assert got == 6 * hw
    zbits = dst[:hw, brd + 4 * hw:].copy().view(np.uint32).ravel()
    last = np.array([z_last], np.float32).view(np.uint32)[0]
    assert all(zbits[p] == (last ^ (0x80000000 if (hw - 1 - p) & 1 else 0)) for p in range(hw))  # the sign of zero included
    assert np.array_equal(dst[:got], want)
    assert (dst[got:] == FILL).all()
    eng.close()


# ---- 6: rejections: OMOK_ERR_INVALID, nothing written ----
def test_rejected_calls_write_nothing():
    n = 9
    hw, brd, rec = _layout(n)
    eng = oa.Engine(board_size=n, games=1, max_nodes=64, max_tables=32, max_batch_k=8)
    src, _ = _synthetic(n, 3, 4, np.float32(1.0), seed=1)  # 12 records: games of 4 at 0, 4, 8
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((6 * 12 * rec,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = {
        "a length of -1 (a game that never finished)": ([0, 4, 8], [4, -1, 4], "game 1"),
        "a length of N*N + 1": ([0, 4, 8], [4, 4, hw + 1], "game 2"),
        "offset + length beyond n_records": ([0, 4, 9], [4, 4, 4], "game 2"),
        "a negative offset": ([-1, 4, 8], [4, 4, 4], "game 0"),
        "games = 0": ([], [], "games"),
    }
    for what, (offs, lens, names) in bad.items():
        with pytest.raises(B.OmokError) as ei:
            eng.replay_augment_records(d_src.data_ptr(), 12, offs, lens, d_dst.data_ptr(), 72)
        assert ei.value.code == ERR_INVALID, what
        assert names in str(ei.value), (what, str(ei.value))  # the message names the first offending game
        torch.cuda.synchronize()
        assert bool((d_dst == FILL).all()), what
    assert eng.replay_augment_records(d_src.data_ptr(), 12, [0, 4, 8], [4, 4, 4], d_dst.data_ptr(), 72) == 72  # the same buffers are accepted when the arguments are right
    eng.close()

"""GPU test of k_tail_fused (fc1 and the heads of whole-K rounds in one launch: the h1 tile goes from fc1's accumulators to the heads' B operand through LDS,
in chunks of eight k-steps, and never to memory).  It must return the bits of the two-launch tail, which OMOK_GEMM_W=1 still selects (k_gemm_w, pinned to
k_gemm_t's bits by test_gpu_tail_gemm.py): every fc1 and heads accumulator sums the same products in the same order.  Batches above 16384 rows take the whole-K
branch (forward_f16x3: tsplit == 1); the shapes are the smallest on it: 16385 rows (129 tiles, the last holding one sample) and 16384 + 128 + 37 (a partly
filled last tile behind full ones)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import omok_ai_amd as oa
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GAMES, K = 1040, 16  # 16640 rows per round: the whole-K branch


@contextmanager
def _gemm_w(value):
    """OMOK_GEMM_W is read at every forward: one process runs both paths"""
    old = os.environ.get("OMOK_GEMM_W")
    try:
        if value is None:
            os.environ.pop("OMOK_GEMM_W", None)
        else:
            os.environ["OMOK_GEMM_W"] = value
        yield
    finally:
        if old is None:
            os.environ.pop("OMOK_GEMM_W", None)
        else:
            os.environ["OMOK_GEMM_W"] = old


def _inputs(n, rows, seed):
    rng = np.random.default_rng(seed)
    hw = n * n
    dens = rng.random((rows, 1)) * 0.6
    u = rng.random((rows, hw))
    board = np.where(u < dens / 2, 1, np.where(u < dens, 2, 0))
    x = np.zeros((rows, 3 * hw), dtype=np.float32)
    x[:, 0:2 * hw:2] = board == 1
    x[:, 1:2 * hw:2] = board == 2
    x[:, 2 * hw:] = rng.integers(0, 2, (rows, 1))
    return x


@pytest.fixture(scope="module", params=[15, 9])
def net(request):
    n = request.param
    tensors = oa.weights.init_random(n, seed=3)
    eng = oa.Engine(board_size=n, games=GAMES, max_nodes=16, max_tables=8, max_batch_k=K)
    eng.load_weights(tensors)
    yield n, tensors, eng
    eng.close()


@pytest.mark.parametrize("rows", [16385, 16384 + 128 + 37])
def test_fused_tail_returns_the_bits_of_the_two_launch_tail(net, rows):
    n, tensors, eng = net
    x = _inputs(n, rows, 11)
    with _gemm_w(None):
        lg_f, vp_f = eng.evaluate_logits(x)
        p_f, v_f = eng.evaluate_pv(x)
        assert eng.last_plan()["tsplit"] == 1, "the batch must take the whole-K branch"
    with _gemm_w("1"):
        lg_w, vp_w = eng.evaluate_logits(x)
        p_w, v_w = eng.evaluate_pv(x)
    assert lg_f.shape[0] == rows and np.isfinite(lg_f).all()
    assert np.array_equal(lg_f, lg_w) and np.array_equal(vp_f, vp_w), "k_tail_fused logits differ from the two-launch tail's"
    assert np.array_equal(p_f, p_w) and np.array_equal(v_f, v_w)
    sel = np.r_[0:64, rows - 64:rows]
    pc, vc = O.Net(n, tensors).forward(x[sel], threads=8)
    assert np.abs(p_f.reshape(rows, -1)[sel] - pc).max() < 1e-3 and np.abs(v_f.reshape(-1)[sel] - vc).max() < 1e-3


def _one_ply(gemm_w):
    """one ply of 64 simulations on 1040 games of 15x15, K = 16: every round is 16640 rows (the fused branch, k_softmax_scatter_policy behind it)"""
    with _gemm_w(gemm_w):
        eng = oa.Engine(board_size=15, games=GAMES, max_nodes=128, max_tables=64, max_batch_k=K, seed=5)
        eng.load_weights(oa.weights.init_random(15, seed=3))
        sp = oa.SelfPlay(eng)
        sp.reset()
        sp.execute(64, K)
        plan = eng.last_plan()
        root_n, root_w = sp.root_stats()
        pi, has = sp.compute_policy()
        moves = sp.sample_actions(1.0, 30)
        eng.close()
    return plan, root_n, root_w, pi, has, moves


def test_one_ply_of_search_is_the_same_with_either_tail():
    plan_f, n_f, w_f, pi_f, has_f, mv_f = _one_ply(None)
    plan_w, n_w, w_w, pi_w, has_w, mv_w = _one_ply("1")
    assert plan_f["tsplit"] == 1 and plan_f["rows"] == GAMES * K and plan_f == plan_w
    assert has_f.all() and (n_f > 0).all()
    assert np.array_equal(mv_f, mv_w), "sampled moves differ"
    assert np.array_equal(n_f, n_w) and np.array_equal(w_f.view(np.uint32), w_w.view(np.uint32))
    assert np.array_equal(has_f, has_w) and np.array_equal(pi_f.view(np.uint32), pi_w.view(np.uint32))

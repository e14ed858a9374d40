"""Nets whose outputs are known in closed form: the policy-head and value-head weight matrices (tensors 29 and 27) are zero, so
logits = p_fc0_b and vpre = v_fc0_b for EVERY position, in every net mode and on every forward path (0 * h + b is exact while h is
finite).  The other 27 tensors are weights.init_random's.  Only L in {0, -200} and b in {0, +-20} are used, which keeps the expected
outputs independent of any expf / tanhf implementation: exp(0) = 1, exp(-200) underflows to 0 in fp32 (1.4e-87 in float64, which the
conversion to fp32 takes to 0), the division is correctly rounded, and tanh(+-20) rounds to +-1 in fp32 and in float64.

  flat        L = 0, b = 0:     p = 1/HW everywhere, v = +0.0: every evaluated sibling ties and q = +0 throughout
  sparse      L = 0 on six spread-out cells, -200 elsewhere, b = +20:  p is exactly 1/6 or 0 and v exactly 1; once the six cells are
              occupied every new row's legal sum is 0
  sparse_neg  the same cells, b = -20: v exactly -1

A search on such a net can be played by the oracle on the analytic rows alone, so the engine's run loop (SelfPlay.run, the path
bench.py times) gets a yardstick that never sees a GPU value."""
import numpy as np

KINDS = ("flat", "sparse", "sparse_neg")
POLICY_W, POLICY_B, VALUE_W, VALUE_B = 29, 30, 27, 28


def sparse_cells(n):
    """six cells spread over the board, no five of which can lie on one line"""
    pts = [(1, 1), (1, n - 3), (n // 2, n // 2 - 1), (n // 2 + 1, n - 2), (n - 2, 2), (n - 3, n // 2 + 1)]
    cells = sorted(y * n + x for y, x in pts)
    assert len(set(cells)) == 6
    return cells


def head_biases(n, kind):
    """(logits L [HW], value bias b) float32"""
    hw = n * n
    if kind == "flat":
        return np.zeros(hw, dtype=np.float32), np.float32(0.0)
    L = np.full(hw, -200.0, dtype=np.float32)
    L[sparse_cells(n)] = 0.0
    return L, np.float32({"sparse": 20.0, "sparse_neg": -20.0}[kind])


def make(n, kind, seed=0):
    from omok_ai_amd import weights
    t = weights.init_random(n, seed=seed)
    L, b = head_biases(n, kind)
    t[POLICY_W] = np.zeros_like(t[POLICY_W])
    t[VALUE_W] = np.zeros_like(t[VALUE_W])
    t[POLICY_B] = L.copy()
    t[VALUE_B] = np.array([b], dtype=np.float32)
    return t


def expected(n, kind, dtype=np.float32):
    """(p [HW], v) float32 of every position: softmax(L) and tanh(b) computed in `dtype`, then rounded to fp32"""
    L, b = head_biases(n, kind)
    L = L.astype(dtype)
    e = np.exp(L - L.max())
    p = (e / e.sum(dtype=dtype)).astype(np.float32)
    v = np.float32(np.tanh(dtype(b)))
    return p, v


def expected_rows(n, kind, count):
    p, v = expected(n, kind)
    return np.tile(p, (count, 1)), np.full(count, v, dtype=np.float32)


def oracle_episode(n, kind, games, count, k, max_plies, seed, game_offset, epsilon=0.25, alpha=0.03, temperature=1.0, threshold=30,
                   cap_nodes=2048, cap_tables=1024, literal=False, collect=None):
    """The arena oracle played step by step on the analytic rows alone (no net, no GPU): returns the O.SelfPlay after max_plies plies
    (0: whole games).  literal: the literal oracle runs alongside and must agree in every bit (test_oracle_literal's _compare).
    collect(dumps): called with the side to move's dumps after every ply's simulations."""
    from oracle import oracle as O
    p1, v1 = expected(n, kind)
    A = O.SelfPlay(n, games, cap_nodes=cap_nodes, cap_tables=cap_tables, seed=seed, game_offset=game_offset)
    A.reset(p1)
    L = None
    if literal:
        from test_oracle_literal import _compare
        L = O.Literal(n, games, seed=seed, game_offset=game_offset, cap_nodes=cap_nodes)
        L.reset(p1)
    ply = 0
    while A.alive_count > 0 and (max_plies == 0 or ply < max_plies):
        for rnd in range((count + k - 1) // k):
            x = A.round_generate(rnd, k, epsilon, alpha)
            p, v = expected_rows(n, kind, len(x))
            A.round_scatter(p, v)
            if L:
                xl, _ = L.round_generate(rnd, k, epsilon, alpha)
                assert len(xl) == len(x)
                L.round_scatter(p, v)  # (every row is the same row: the slot order does not matter)
        assert A.error == 0
        if collect:
            collect([A.tree_dump(g, ply & 1) for g in range(games) if A.game_alive(g)])
        acts = A.sample(temperature, threshold)
        m = A.mirror_generate()
        pm, _ = expected_rows(n, kind, len(m))
        if L:
            _compare(A, L, games, f"{kind}: ply {ply} after execute")
            assert np.array_equal(acts, L.sample(temperature, threshold))
            assert len(L.mirror_generate()[0]) == len(m)
            L.advance(pm)
        A.advance(pm)
        assert A.error == 0 and (L is None or L.error == 0)
        if L:
            _compare(A, L, games, f"{kind}: ply {ply} after advance")
        ply += 1
    if L:
        for g in range(games):
            assert A.game_status(g) == L.game_status(g) and A.game_plies(g) == L.game_plies(g)
            for a, b in zip(A.replay(g), L.replay(g)):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return A


# the run-loop cases of tests/test_gpu_head_bias_nets.py: (kind, board, games, sims, K, plies, mode name, engine seed); the seeds are
# chosen so that the ORACLE episode meets the coverage floors (tests/test_head_bias_nets.py)
RUN_CASES = [
    ("flat", 9, 8, 32, 8, 0, "mixed", 22),
    ("sparse", 9, 8, 32, 8, 0, "mixed", 22),
    ("sparse_neg", 9, 8, 32, 8, 0, "mixed", 22),
    ("flat", 15, 8, 64, 16, 12, "default", 22),
    ("sparse", 15, 8, 64, 16, 12, "default", 22),
]
GAME_OFFSET = 5
THRESHOLD = 99  # Boltzmann on every ply: games of near-uniform moves last long enough for roots with fewer empty cells than simulations
FLOOR_KEYS = {"flat": ("tie_nodes", "signed_zero_w_pos"), "sparse": ("zero_rows", "zero_p_legal", "saturated_w"),
              "sparse_neg": ("zero_rows", "zero_p_legal", "saturated_w")}


def floor_keys(kind, n, count, plies):
    """FLOOR_KEYS less what a run of SelfPlay.run from a fresh reset cannot reach in `plies` plies: tie_nodes and saturated_w where PUCT never
    runs (adversarial_outputs.puct_reachable: the two board-15 cases of 12 plies); zero_rows needs the six cells occupied, which 12 plies of a
    225-cell board do not bring about"""
    from adversarial_outputs import puct_reachable
    keys = [k for k in FLOOR_KEYS[kind] if puct_reachable(n, count, plies) or k not in ("tie_nodes", "saturated_w")]
    return [k for k in keys if plies == 0 or k != "zero_rows"]

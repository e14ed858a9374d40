"""Net outputs no random-init net emits, for the search-parity tests (plain numpy, no GPU, no product import).

rows() / mirror_rows() make up the (p, v) of one request batch: exact ties, rows whose legal mass is 0, denormal, exactly
2^-23 or one ulp below it, zeros on legal cells, huge unnormalised rows, and values of +-1, +-0 and the smallest denormal.
puct_scores() restates the oracle's PUCT on a canonical tree dump and coverage() counts, over a list of dumps, how often each
of the branches those rows aim at was actually taken, so that a test can demand that they were.

Every value is FINITE.  NaN and +-inf are out of scope: f32::total_cmp orders NaNs by sign and payload, and the sign of an
arithmetic NaN (0 * inf, inf - inf) differs between x86 and gfx950, so no yardstick exists for them; a net with finite weights
emits none.  One consequence: with epsilon = 0 the root row is renormalised WITHOUT the EPS rule (pme.rs:63-68), so a root whose
legal mass is 0 or denormal turns into NaN / inf there.  Only a node of the side to move can ever be a searched root: a mirror row (it
becomes the other tree's root at once) or a request at even depth.  Configurations that run without noise pass finite_roots as a mask
over the batch (root_candidates) and only those rows are replaced by the exact-uniform row; requests at odd depth keep every kind.
"""
import numpy as np

EPS = np.float32(2.0 ** -23)
TINY = np.float32(2.0 ** -149)       # the smallest fp32 denormal
MIN_NORMAL = np.float32(2.0 ** -126)
FLOOR = 10                           # every coverage count a configuration can reach must be at least this

KINDS = ("uniform", "dyadic", "onehot_empty", "onehot_occupied", "zero", "denormal", "eps_one", "eps_two", "eps_one_marked",
         "eps_two_marked", "below_eps", "huge", "softmax", "repeat")
# weights of the draw: repeats and dyadic rows (ties) and the rows the EPS rule decides carry most of it
KIND_WEIGHTS = np.array([2, 4, 2, 2, 2, 3, 1, 1, 2, 2, 2, 1, 2, 6], dtype=np.float64)
# black_wins / white_wins: +-1 by the side to move, as a net sure of the game's result would say; along a line of such values every backup into a
# node has the same sign after the negation per level, which is what makes |w| = n >= 2
VALUE_KINDS = ("+1", "-1", "+0", "-0", "+0.5", "-0.5", "+0.25", "-0.25", "tiny", "-tiny", "uniform", "black_wins", "white_wins")
VALUE_WEIGHTS = np.array([3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 2, 10, 10], dtype=np.float64)
_FIXED_VALUES = [1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 0.25, -0.25, float(TINY), -float(TINY)]

# (name, board, games, sims, K, plies (0: whole games), settings): the cases of tests/test_gpu_injected_outputs.py, which
# tests/test_adversarial_outputs.py runs on the two oracles alone.  kind_seed is chosen so that the ORACLE meets the floors.
CASES = [
    ("n9_whole_games", 9, 6, 32, 8, 0, {"kind_seed": 4, "seed": 90, "threshold": 99}),
    ("n15_k16", 15, 4, 48, 16, 16, {"kind_seed": 7, "opening": 225 - 20}),
    ("n9_k1", 9, 3, 12, 1, 10, {"kind_seed": 72, "opening": 81 - 11}),
    ("n9_no_noise", 9, 4, 24, 8, 12, {"kind_seed": 10, "epsilon": 0.0, "temperature": 0.5, "threshold": 4, "opening": 81 - 16}),
]
# opening: that many moves of helpers.draw_sequence (a fill of the board that never makes a five) are played first as external moves
# (set_actions, mirror rows injected as everywhere), so that the case's searched plies start on a board with no more empty cells than a ply
# has simulations (and enough of them for the case's plies): every root is then fully expanded and PUCT runs between visited children at
# these shapes too (see puct_reachable).  select() stops at a node that is not fully expanded, so from an empty board these cases' few plies
# would never reach PUCT.


def puct_reachable(n, count, plies, opening=0):
    """Can PUCT run at all in this configuration?  select() stops at the first node that is not fully expanded (node.rs:43-58),
    and the root of a tree that has never been fully expanded starts each of its own plies without children (no simulation went past
    its parent), so it gains at most `count` children per ply: until the board has no more than `count` empty cells, every simulation
    expands a child of the root, no node is ever fully expanded and no child is visited twice.  tie_nodes and saturated_w (n >= 2) are
    then 0 by arithmetic, whatever the rows."""
    return plies == 0 or count >= n * n - opening - (plies - 1)


def occupied_cells(inputs):
    """[n][HW] bool from the encoder layout [n][3 HW]: cell i has its two stone planes at 2 i, 2 i + 1 (encoder.rs:22-43)"""
    inputs = np.asarray(inputs, dtype=np.float32)
    hw = inputs.shape[1] // 3
    return inputs[:, :2 * hw].reshape(len(inputs), hw, 2).sum(axis=2) > 0


def f32_sum(x):
    """the sequential float32 sum over the cells ascending (what mask-and-renormalise computes)"""
    x = np.asarray(x, dtype=np.float32)
    return np.float32(0.0) if x.size == 0 else np.cumsum(x, dtype=np.float32)[-1]


def _row(kind, rng, occ, prev):
    hw = len(occ)
    empty = np.flatnonzero(~occ)
    full = np.flatnonzero(occ)
    p = np.zeros(hw, dtype=np.float32)
    if kind == "repeat":
        return None if prev is None else prev.copy()
    if kind == "uniform":
        p[:] = 1.0
    elif kind == "dyadic":
        m = min(len(empty), int(rng.integers(2, 6)))
        p[rng.choice(empty, m, replace=False)] = rng.integers(1, 5, m).astype(np.float32) * np.float32(2.0 ** -10)
        if len(full):
            p[rng.choice(full)] = np.float32(0.5)  # mass the mask removes
    elif kind == "onehot_empty":
        p[rng.choice(empty)] = 1.0
    elif kind == "onehot_occupied":
        if len(full):
            p[rng.choice(full)] = 1.0
    elif kind == "zero":
        pass
    elif kind == "denormal":
        p[full] = np.float32(1.0) / np.float32(max(1, len(full)))
        m = int(rng.integers(1, len(empty) + 1))
        p[rng.choice(empty, m, replace=False)] = rng.choice(np.array([1e-40, 1e-41, 1e-42, 1e-43, 1e-44], dtype=np.float32), m)
    elif kind in ("eps_one", "eps_one_marked", "eps_two", "eps_two_marked"):
        # legal sum exactly 2^-23: one cell of 2^-23, or two of 2^-24.  The marked variants add the smallest denormal on one more
        # empty cell: the fp32 sum absorbs it (ulp(2^-23) = 2^-46), so the sum is still exactly 2^-23, and the renormalised row holds
        # 2^-149 * 2^23 = 2^-126 there, which no other kind produces: the stored row then proves which side of the rule was taken
        two = kind.startswith("eps_two") and len(empty) >= 2
        marked = kind.endswith("marked") and len(empty) >= (3 if two else 2)
        cells = rng.choice(empty, (2 if two else 1) + (1 if marked else 0), replace=False)
        if two:
            p[cells[:2]] = np.float32(2.0 ** -24)
        else:
            p[cells[0]] = EPS
        if marked:
            p[cells[-1]] = TINY
        if len(full):
            p[rng.choice(full)] = np.float32(0.75)
    elif kind == "below_eps":
        p[rng.choice(empty)] = np.nextafter(EPS, np.float32(0.0))
        if len(full):
            p[rng.choice(full)] = np.float32(0.75)
    elif kind == "huge":
        p[:] = (rng.uniform(0.5, 1.5, hw) * 1e30).astype(np.float32)
    elif kind == "softmax":
        z = rng.standard_normal(hw) * 2.0
        e = np.exp(z - z.max())
        p[:] = (e / e.sum()).astype(np.float32)
    else:
        raise ValueError(kind)
    return p


def _value(rng, black_to_move):
    k = int(rng.choice(len(VALUE_KINDS), p=VALUE_WEIGHTS / VALUE_WEIGHTS.sum()))
    u = rng.uniform(-1.0, 1.0)  # (drawn always: the stream does not depend on the kind)
    if VALUE_KINDS[k] in ("black_wins", "white_wins"):
        return np.float32(1.0 if black_to_move == (VALUE_KINDS[k] == "black_wins") else -1.0)
    return np.float32(_FIXED_VALUES[k]) if k < len(_FIXED_VALUES) else np.float32(u)


def _batch(stream, inputs, finite_roots, with_values):
    occ = occupied_cells(inputs)
    n, hw = occ.shape
    finite_roots = np.broadcast_to(np.asarray(finite_roots, dtype=bool), (n,))
    turn_plane = np.asarray(inputs, dtype=np.float32)[:, 2 * hw] > 0 if n else np.zeros(0, dtype=bool)  # Black to move (encoder.rs: the third plane)
    rng = np.random.default_rng(stream)
    p = np.zeros((n, hw), dtype=np.float32)
    v = np.zeros(n, dtype=np.float32)
    prev = None
    for r in range(n):
        kind = KINDS[int(rng.choice(len(KINDS), p=KIND_WEIGHTS / KIND_WEIGHTS.sum()))]
        sub = np.random.default_rng(rng.integers(0, 2 ** 63))  # (a row's own stream: the kinds draw different amounts)
        val = _value(sub, bool(turn_plane[r]))
        if occ[r].all():  # (a full board is never requested: a game ends with its last cell)
            kind = "zero"
        row = _row(kind, sub, occ[r], prev)
        if row is None:
            row = _row("softmax", sub, occ[r], None)
        elif kind == "repeat":
            val = v[r - 1]
        if finite_roots[r] and not f32_sum(np.where(occ[r], np.float32(0.0), row)) >= np.float32(2.0 ** -24):
            row = _row("uniform", sub, occ[r], None)
        p[r], v[r] = row, val
        prev = row
    assert np.isfinite(p).all() and np.isfinite(v).all()
    return (p, v) if with_values else p


def rows(kind_seed, ply, rnd, inputs, finite_roots=False):
    """(p [n][HW], v [n]) float32 for the request batch `inputs` [n][3 HW] of round `rnd` of ply `ply`: deterministic in its
    arguments; the kind is drawn per request and the row is built relative to that request's own board."""
    return _batch([int(kind_seed), int(ply), int(rnd), 0], inputs, finite_roots, True)


def mirror_rows(kind_seed, ply, inputs, finite_roots=False):
    """p [n][HW] for the mirror batch of ply `ply` (the boards AFTER the move: the move's cell counts as occupied)"""
    return _batch([int(kind_seed), int(ply), 0, 1], inputs, finite_roots, False)


def root_candidates(osp, side, nreq):
    """mask over the current request batch of `osp` (an oracle SelfPlay): True for requests at even depth, the only ones that can become the
    root of a searched tree (a tree is searched when its own side is to move)"""
    out = np.zeros(nreq, dtype=bool)
    depth_of = {}
    for r in range(nreq):
        g, node = osp.request_info(r)
        if g not in depth_of:
            parent = osp.tree_dump(g, side)[0][:, 0]
            depth = np.zeros(len(parent), dtype=np.int64)
            for i in range(1, len(parent)):
                depth[i] = depth[parent[i]] + 1
            depth_of[g] = depth
        out[r] = depth_of[g][node] % 2 == 0
    return out


def legal_sums(p, inputs):
    occ = occupied_cells(inputs)
    return np.array([f32_sum(np.where(occ[r], np.float32(0.0), p[r])) for r in range(len(p))], dtype=np.float32)


def without_eps_rule(p, inputs):
    """what "a kernel without the EPS rule" would store: the legal cells of rows with 0 < legal sum < 2^-23 pre-divided by that sum"""
    p = np.array(p, dtype=np.float32)
    occ = occupied_cells(inputs)
    s = legal_sums(p, inputs)
    for r in np.flatnonzero((s > 0) & (s < EPS)):
        p[r, ~occ[r]] = p[r, ~occ[r]] / s[r]
    assert np.isfinite(p).all()
    return p


def flush_denormals(x):
    """what "a kernel with FTZ" would read: denormals become (signed) zero"""
    x = np.array(x, dtype=np.float32)
    return np.where(np.abs(x) < MIN_NORMAL, np.copysign(np.float32(0.0), x), x).astype(np.float32)


def puct_scores(ints, floats, node):
    """The oracle's PUCT (oracle/selfplay.c: run_sim's selection loop) restated in float32 numpy on a canonical tree dump:
    (child node indices in insertion-rank order, their scores float32, their f32::total_cmp keys int32).  Every operation is one
    correctly rounded float32 operation, as in the C compiled without contraction."""
    ints = np.asarray(ints)
    kids = np.flatnonzero(ints[:, 0] == node)
    kids = kids[np.argsort(ints[kids, 7] & 0xFFFF, kind="stable")]
    parent_n = np.float32(max(int(ints[node, 6]) & 0xFFFFFFFF, 1))
    sq = np.sqrt(parent_n, dtype=np.float32)
    n = ints[kids, 6].astype(np.uint32)
    w = floats[kids, 0].astype(np.float32)
    p = floats[node, 1 + ints[kids, 1]].astype(np.float32)
    q = w / (n.astype(np.float32) + EPS)
    bias = sq / (np.uint32(1) + n).astype(np.float32)
    score = (q + (np.float32(1.0) * p) * bias).astype(np.float32)
    b = score.view(np.int32)
    keys = b ^ ((b >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)
    return kids, score, keys


def first_and_last_max(keys):
    """(index of the first maximum, index of the last maximum): Iterator::max_by returns the LAST"""
    m = keys.max()
    at = np.flatnonzero(keys == m)
    return int(at[0]), int(at[-1])


def coverage(dumps):
    """Counts over a list of canonical tree dumps [(ints, floats), ...]:
      tie_nodes         fully expanded nodes whose maximal PUCT score is shared by >= 2 children with n > 0
      unnormalised_rows has_policy = 1, legal > 0, stored row sum < 2^-23; = zero_rows + denormal_rows + below_eps_rows
      zero_rows           ... the row is all zero
      denormal_rows       ... every non-zero entry is an fp32 denormal
      below_eps_rows      ... the rest (a normal number below 2^-23: the row one ulp under the threshold)
      eps_exact_rows    rows that prove the <= side at sum = 2^-23: they hold 2^-126 (the renormalised marker denormal) beside one entry
                        of 1 or two of 1/2 (had the rule been <, the row would hold 2^-149 beside 2^-23 / 2^-24 and is not counted)
      zero_p_legal      nodes with a child (a legal cell) whose prior is exactly 0 while the row has non-zero entries: score = q alone
      saturated_w       children with |w| == n >= 2 (every backup through them was +1, or every one -1)
      signed_zero_w_pos / _neg   children with n > 0 and w == +0.0 / -0.0"""
    out = dict.fromkeys(("tie_nodes", "unnormalised_rows", "zero_rows", "denormal_rows", "below_eps_rows", "eps_exact_rows", "zero_p_legal",
                         "saturated_w", "signed_zero_w_pos", "signed_zero_w_neg"), 0)
    for ints, floats in dumps:
        if len(ints) == 0:
            continue
        has = (ints[:, 7] >> 16) & 1
        legal, nch, n = ints[:, 4], ints[:, 5], ints[:, 6]
        row = floats[:, 1:]
        s = row.astype(np.float64).sum(axis=1)
        un = (has == 1) & (legal > 0) & (s < float(EPS))
        nz = row != 0
        den = un & (s > 0) & ~(nz & (np.abs(row) >= MIN_NORMAL)).any(axis=1)
        out["unnormalised_rows"] += int(un.sum())
        out["zero_rows"] += int((un & (s == 0)).sum())
        out["denormal_rows"] += int(den.sum())
        out["below_eps_rows"] += int((un & (s > 0) & ~den).sum())
        cnt = nz.sum(axis=1)
        marker = (row == MIN_NORMAL).sum(axis=1) == 1
        one = ((row == 1.0).sum(axis=1) == 1) & (cnt == 2)
        two = ((row == 0.5).sum(axis=1) == 2) & (cnt == 3)
        out["eps_exact_rows"] += int(((has == 1) & marker & (one | two)).sum())
        child = ints[:, 0] >= 0
        w = floats[:, 0]
        out["saturated_w"] += int((child & (n >= 2) & (np.abs(w) == n.astype(np.float32))).sum())
        zero_w = child & (n > 0) & (w == 0)
        neg = np.signbit(w)
        out["signed_zero_w_pos"] += int((zero_w & ~neg).sum())
        out["signed_zero_w_neg"] += int((zero_w & neg).sum())
        par = ints[child, 0]
        prior = row[par, ints[child, 1]]
        zp = np.zeros(len(ints), dtype=bool)
        zp[par[(prior == 0) & (cnt[par] > 0)]] = True
        out["zero_p_legal"] += int(zp.sum())
        for node in np.flatnonzero((nch == legal) & (nch > 0)):
            out["tie_nodes"] += is_tie_node(ints, floats, int(node))
    return out


def is_tie_node(ints, floats, node):
    kids, _, keys = puct_scores(ints, floats, node)
    top = keys == keys.max()
    return bool((top & (ints[kids, 6] > 0)).sum() >= 2)


def add_counts(a, b):
    return {k: a.get(k, 0) + b[k] for k in b}


def floor_keys(n, count, plies, epsilon=0.25, opening=0):
    """The coverage counts the floor applies to in a configuration: all of them, except those the configuration cannot reach by
    construction: tie_nodes and saturated_w where PUCT never runs (puct_reachable; none of CASES), and signed_zero_w_neg everywhere: a w starts
    as +0.0 and x + (-0.0) is -0.0 only for x = -0.0, so v = +0.0 (value = -0.0) leaves w = +0.0 and q = +0.0; the count is kept to
    show it (a kernel that accumulated w otherwise would differ from the oracle in the dump's bits)."""
    keys = ["unnormalised_rows", "zero_rows", "denormal_rows", "below_eps_rows", "eps_exact_rows", "zero_p_legal", "signed_zero_w_pos"]
    return keys + (["tie_nodes", "saturated_w"] if puct_reachable(n, count, plies, opening) else [])

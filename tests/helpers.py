"""Shared helpers of the parity tests (the drivers import the product and the oracle when they are called)."""
import numpy as np


def draw_sequence(n):
    """A legal move sequence that fills the whole n x n board (n in {9, 15}) without ever making an exact five:
    cell (x, y) is Black iff ((x + 2y + off) mod 4) >= 2 -- every row, column and diagonal has runs of at most 2 / 4 -- and
    Black owns one cell more than White, so alternating moves use the cells up exactly.  The last move ends the game as
    GameStatus::Draw (environment/src/lib.rs:160-161)."""
    off = {9: 2, 15: 1}[n]
    black = [y * n + x for y in range(n) for x in range(n) if ((x + 2 * y + off) % 4) >= 2]
    white = [y * n + x for y in range(n) for x in range(n) if ((x + 2 * y + off) % 4) < 2]
    assert len(black) == len(white) + 1
    seq = []
    for i in range(len(white)):
        seq += [black[i], white[i]]
    seq.append(black[-1])
    return seq


def tree_shape(ints):
    """(fully expanded nodes, fully expanded non-root nodes, max depth) of a canonical tree dump
    (ints [n][8] = parent, action, status, turn, legal, nch, n, order|has_policy<<16)."""
    parent, legal, nch = ints[:, 0], ints[:, 4], ints[:, 5]
    full = (nch == legal) & (nch > 0)
    depth = np.zeros(len(ints), dtype=np.int64)
    for i in range(1, len(ints)):
        depth[i] = depth[parent[i]] + 1  # creation order: parent index < child index
    return int(full.sum()), int(full[1:].sum()), int(depth.max()) if len(ints) else 0


def random_positions(n, count, seed):
    """`count` positions in the encoder.rs input layout [count][3 n n]: random stones (0 .. n*n - 2 of them) placed through the
    oracle's rules, random side to move."""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    out = np.zeros((count, 3 * n * n), dtype=np.float32)
    for i in range(count):
        env = O.Environment(n)
        for c in rng.permutation(n * n)[: int(rng.integers(0, n * n - 1))]:
            env.place_stone(int(c))
        out[i] = env.encode_nn_input(int(rng.integers(0, 2)))
    return out


def compare_trees(sp, osp, games, tag):
    for g in range(games):
        for side in (0, 1):
            gi, gf = sp.tree_dump(g, side)
            oi, of = osp.tree_dump(g, side)
            assert gi.shape == oi.shape, f"{tag}: game {g} side {side}: {gi.shape[0]} vs {oi.shape[0]} nodes"
            assert np.array_equal(gi, oi), f"{tag}: node records differ (game {g} side {side})"
            assert np.array_equal(gf.view(np.uint32), of.view(np.uint32)), f"{tag}: w/policy bits differ (game {g} side {side})"
            assert sp.tree_root(g, side)[0] == osp.tree_root(g, side)[0]
            assert np.float32(sp.tree_root(g, side)[1]).tobytes() == np.float32(osp.tree_root(g, side)[1]).tobytes()


def drive_selfplay_vs_oracle(n, games, count, k, max_plies, mode, threshold=6, max_nodes=2048, max_tables=1024, seed=7,
                             game_offset=5, weight_seed=0, epsilon=0.25, alpha=0.03, temperature=1.0, on_sample=None, tensors=None):
    """Plays `games` games step by step on the engine and on the oracle (the oracle consumes the GPU net's p / v, so the
    comparison isolates the tree arithmetic) and compares canonical tree dumps, request boards, moves and replay tuples bit
    for bit.  Returns the shape of the deepest search seen by the ORACLE: (fully expanded nodes, fully expanded non-root
    nodes, max depth, max tables) so that a test can prove it left the shallow root-plus-one-layer regime.
    on_sample(ply, pi [games][hw], has [games], actions [games]): called with the engine's compute_policy read BEFORE the
    ply's sample_actions and the moves that call chose.  tensors: the net's 31 tensors, in place of the random-init net `weight_seed`."""
    import omok_ai_amd as oa
    from oracle import oracle as O
    if tensors is None:
        tensors = oa.weights.init_random(n, seed=weight_seed)
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed,
                    game_offset=game_offset, net_mode=mode)
    eng.load_weights(tensors)
    sp = oa.SelfPlay(eng)
    sp.reset()
    root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=max_nodes, cap_tables=max_tables, seed=seed, game_offset=game_offset)
    osp.reset(root_p)
    compare_trees(sp, osp, games, "reset")
    shape = [0, 0, 0, 0]
    ply = 0
    rounds = (count + k - 1) // k
    while osp.alive_count > 0 and (max_plies == 0 or ply < max_plies):
        for rnd in range(rounds):
            nreq = sp.round_generate(rnd, k, epsilon, alpha)
            oin = osp.round_generate(rnd, k, epsilon, alpha)
            assert nreq == len(oin), f"ply {ply} round {rnd}: request count"
            assert np.array_equal(sp.round_inputs(), oin), f"ply {ply} round {rnd}: request boards"
            if rnd == 0 or (rounds > 20 and rnd % 16 == 15):  # pending children of the round are in the dump as well
                compare_trees(sp, osp, games, f"ply {ply} after generate of round {rnd}")
            p, v = sp.round_eval()
            sp.round_scatter()
            osp.round_scatter(p, v)
        compare_trees(sp, osp, games, f"ply {ply} after execute")
        assert osp.error == 0
        for g in range(games):
            if osp.game_alive(g):
                full, full_nr, depth = tree_shape(osp.tree_dump(g, ply & 1)[0])
                shape = [max(shape[0], full), max(shape[1], full_nr), max(shape[2], depth), max(shape[3], osp.tree_root(g, ply & 1)[3])]
        if on_sample is not None:
            pi, has = sp.compute_policy()
            pi, has = np.array(pi).copy(), np.array(has).copy()
        a = sp.sample_actions(temperature, threshold)
        assert np.array_equal(a, osp.sample(temperature, threshold)), f"ply {ply}: actions"
        if on_sample is not None:
            on_sample(ply, pi, has, np.array(a))
        nm = sp.mirror_generate()
        om = osp.mirror_generate()
        assert nm == len(om) and np.array_equal(sp.mirror_inputs(), om)
        pm = sp.mirror_eval()
        sp.mirror_apply()
        osp.advance(pm)
        compare_trees(sp, osp, games, f"ply {ply} after advance")
        alive, status, plies = sp.game_info()
        assert [int(x) for x in alive] == [osp.game_alive(g) for g in range(games)]
        assert [int(x) for x in status] == [osp.game_status(g) for g in range(games)]
        ply += 1
    assert sp.alive_count == osp.alive_count
    for g in range(games):
        gb, gt, gp, gz = sp.replay(g)
        ob, ot, op, oz = osp.replay(g)
        assert np.array_equal(gb, ob) and np.array_equal(gt, ot) and np.array_equal(gz, oz)
        assert np.array_equal(gp.view(np.uint32), op.view(np.uint32))
    eng.close()
    return tuple(shape)


def drive_injected_vs_oracle(n, games, count, k, max_plies, mode, kind_seed, threshold=6, max_nodes=2048, max_tables=1024, seed=7,
                              game_offset=5, weight_seed=0, epsilon=0.25, alpha=0.03, temperature=1.0, opening=0):
    """drive_selfplay_vs_oracle with the net taken out of the loop: after the reset (whose root row is the net's, as there) neither
    side evaluates anything.  Every round's (p, v) and every mirror batch's p come from tests/adversarial_outputs.py and go into the
    engine through round_inject / mirror_inject and into the oracle as arguments, so the tree kernels meet rows no net emits: exact
    ties, zero and denormal rows, legal sums at and around 2^-23, v = +-1, +-0.  Compared bit for bit at the same points.  Returns the
    coverage counts (adversarial_outputs.coverage) of the ORACLE's dumps of both trees of every live game after every ply's simulations
    and after every advance (each of those dumps has just been compared with the device's, bit for bit).
    opening: that many moves of draw_sequence(n) are played first as external moves (set_actions; their mirror rows are injected
    too), so that the searched plies start on a board with few empty cells and PUCT runs between visited children from the first ply on.
    Without noise only rows that can become a searched root (mirror rows, requests at even depth) are kept finite under the root's
    unguarded renormalisation (adversarial_outputs.root_candidates); every other request keeps every kind."""
    import omok_ai_amd as oa
    import adversarial_outputs as AO
    from oracle import oracle as O
    tensors = oa.weights.init_random(n, seed=weight_seed)
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed,
                    game_offset=game_offset, net_mode=mode)
    eng.load_weights(tensors)
    sp = oa.SelfPlay(eng)
    sp.reset()
    root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=max_nodes, cap_tables=max_tables, seed=seed, game_offset=game_offset)
    osp.reset(root_p)
    compare_trees(sp, osp, games, "reset")
    no_noise = epsilon == 0.0
    counts = {}
    ply = 0
    rounds = (count + k - 1) // k
    for cell in draw_sequence(n)[:opening]:
        acts = np.full(games, cell, dtype=np.int32)
        sp.set_actions(acts)
        osp.set_actions(acts)
        nm = sp.mirror_generate()
        om = osp.mirror_generate()
        assert nm == len(om) == games and np.array_equal(sp.mirror_inputs(), om)
        pm = AO.mirror_rows(kind_seed, ply, om, no_noise)
        sp.mirror_inject(pm)
        sp.mirror_apply()
        osp.advance(pm)
        assert osp.error == 0 and osp.alive_count == games
        ply += 1
    if opening:
        compare_trees(sp, osp, games, "after the opening")
    while osp.alive_count > 0 and (max_plies == 0 or ply - opening < max_plies):
        side = ply & 1
        for rnd in range(rounds):
            nreq = sp.round_generate(rnd, k, epsilon, alpha)
            oin = osp.round_generate(rnd, k, epsilon, alpha)
            assert nreq == len(oin), f"ply {ply} round {rnd}: request count"
            assert np.array_equal(sp.round_inputs(), oin), f"ply {ply} round {rnd}: request boards"
            if rnd == 0 or (rounds > 20 and rnd % 16 == 15):
                compare_trees(sp, osp, games, f"ply {ply} after generate of round {rnd}")
            p, v = AO.rows(kind_seed, ply, rnd, oin, AO.root_candidates(osp, side, len(oin)) if no_noise else False)
            sp.round_inject(p, v)
            sp.round_scatter()
            osp.round_scatter(p, v)
        compare_trees(sp, osp, games, f"ply {ply} after execute")
        assert osp.error == 0
        counts = AO.add_counts(counts, AO.coverage([osp.tree_dump(g, sd) for g in range(games) if osp.game_alive(g) for sd in (0, 1)]))
        a = sp.sample_actions(temperature, threshold)
        assert np.array_equal(a, osp.sample(temperature, threshold)), f"ply {ply}: actions"
        moved = [g for g in range(games) if osp.game_alive(g)]
        nm = sp.mirror_generate()
        om = osp.mirror_generate()
        assert nm == len(om) and np.array_equal(sp.mirror_inputs(), om)
        pm = AO.mirror_rows(kind_seed, ply, om, no_noise)
        sp.mirror_inject(pm)
        sp.mirror_apply()
        osp.advance(pm)
        assert osp.error == 0
        compare_trees(sp, osp, games, f"ply {ply} after advance")
        counts = AO.add_counts(counts, AO.coverage([osp.tree_dump(g, sd) for g in moved if osp.game_alive(g) for sd in (0, 1)]))
        alive, status, plies = sp.game_info()
        assert [int(x) for x in alive] == [osp.game_alive(g) for g in range(games)]
        assert [int(x) for x in status] == [osp.game_status(g) for g in range(games)]
        assert [int(x) for x in plies] == [osp.game_plies(g) for g in range(games)]
        ply += 1
    assert sp.alive_count == osp.alive_count
    for g in range(games):
        gb, gt, gp, gz = sp.replay(g)
        ob, ot, op, oz = osp.replay(g)
        assert np.array_equal(gb, ob) and np.array_equal(gt, ot) and np.array_equal(gz.view(np.uint32), oz.view(np.uint32))
        assert np.array_equal(gp.view(np.uint32), op.view(np.uint32))
    eng.close()
    return counts


def boltzmann_expected(pi, temperature, u):
    """Agent::sample_action(Boltzmann) restated in float64 (agent.rs:106-133): the heated distribution of one policy row and
    the cell a uniform draw u in [0, 1) selects.  Returns (cell, min |q - u| over the cumulative distribution q): a draw
    closer to a step of q than the fp32 rounding of the weights can be moved across it by that rounding."""
    pi = np.asarray(pi, dtype=np.float32)
    arg = pi.astype(np.float64) / np.float64(np.float32(temperature))
    h = np.where(pi >= np.float32(2.0 ** -23), np.exp(arg), 0.0)
    q = np.cumsum(h / h.sum())
    return int(np.searchsorted(q, u, side="right")), float(np.abs(q - u).min())


def sample_uniform(seed, episode, ply, tree_global):
    """the u of the RNG contract's purpose 3 (SAMPLE): (word 0 of Philox(key, 0, ply, tree_global, 3) >> 8) * 2^-24"""
    import ctypes as C
    from oracle import oracle as O
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox(O.stream_key(seed, episode), 0, int(ply), int(tree_global), 3, out)
    return (int(out[0]) >> 8) * 2.0 ** -24


def dirichlet_spread(rows):
    """mean((P - 1/HW)^2) over rows [trees][HW] of Dirichlet draws, and its analytic value for Dirichlet(alpha, ..., alpha) as a
    function of alpha: Var(P_i) = (1/HW)(1 - 1/HW) / (HW alpha + 1)."""
    rows = np.asarray(rows, dtype=np.float64)
    hw = rows.shape[1]
    return float(((rows - 1.0 / hw) ** 2).mean()), lambda alpha: (1.0 / hw) * (1.0 - 1.0 / hw) / (hw * alpha + 1.0)


def dirichlet_spread_sigma(hw, trees, alpha, draws=300):
    """standard deviation of dirichlet_spread's statistic over `draws` samples of `trees` rows from numpy's own Dirichlet"""
    rng = np.random.default_rng(0)
    x = rng.dirichlet(np.full(hw, alpha), size=(draws, trees))
    return float((((x - 1.0 / hw) ** 2).mean(axis=(1, 2))).std(ddof=1))


def check_root_noise(sp, games, hw, alpha, tag):
    """`sp` (the engine's SelfPlay or the oracle's: same tree_dump) has just run round_generate(0, K, epsilon = 1.0, alpha): every
    side-0 root policy row is then a normalised row of Gamma(alpha) draws, i.e. Dirichlet(alpha, ..., alpha).  Checks, against
    numpy's own Dirichlet and the closed forms, not against the oracle (which shares the sampler's design with the kernel):
    rows sum to 1 within 1e-6; the spread statistic within 5 measured standard deviations of its analytic value; at
    alpha = 0.03 the share of exactly-zero entries (draws below the 1e-30 flush) within 5 binomial standard deviations of
    P(Gamma(alpha) < 1e-30) = 1e-30 ** alpha / Gamma(alpha + 1).  Returns the deviation of the spread in sigmas."""
    import math
    rows = np.stack([sp.tree_dump(g, 0)[1][0, 1:] for g in range(games)]).astype(np.float64)
    assert rows.shape == (games, hw)
    assert np.all(rows >= 0.0)
    sums = rows.sum(axis=1)
    assert np.abs(sums - 1.0).max() < 1e-6, f"{tag}: a row sums to {sums[np.abs(sums - 1.0).argmax()]!r}"
    s, analytic = dirichlet_spread(rows)
    sigma = dirichlet_spread_sigma(hw, games, alpha)
    dev = (s - analytic(alpha)) / sigma
    print(f"{tag}: alpha {alpha}: spread {s:.6e}, analytic {analytic(alpha):.6e}, sigma {sigma:.3e}: {dev:+.2f} sigma")
    assert abs(dev) < 5.0, f"{tag}: alpha {alpha}: spread {s!r} is {dev:+.2f} sigma from {analytic(alpha)!r}"
    if alpha == 0.03:
        share = float((rows == 0.0).mean())
        want = 1e-30 ** alpha / math.gamma(1.0 + alpha)
        sd = math.sqrt(want * (1.0 - want) / rows.size)
        print(f"{tag}: alpha {alpha}: share of zero entries {share:.5f}, expected {want:.5f}, sd {sd:.5f}: {(share - want) / sd:+.2f} sd")
        assert abs(share - want) < 5.0 * sd
    return dev


class BoltzmannCheck:
    """on_sample hook of drive_selfplay_vs_oracle (and of the oracle-only driver of tests/test_oracle_net_rng.py): every move a
    live game samples must be the cell boltzmann_expected names for the policy read before the call and the u of the RNG
    contract, unless u lies within 1e-5 of a step of the float64 cumulative distribution (the fp32 weights of the code under
    test may round across it): those samples are skipped and counted."""

    def __init__(self, seed, game_offset, temperature, episode=0):
        self.seed, self.game_offset, self.temperature, self.episode = seed, game_offset, temperature, episode
        self.samples = self.skipped = self.nonuniform = 0
        self.max_arg = 0.0  # the largest pi / T handed to exp
        self.mismatches = []

    def __call__(self, ply, pi, has, actions):
        side = ply & 1
        for g in range(len(actions)):
            if not has[g]:
                assert actions[g] == -1
                continue
            u = sample_uniform(self.seed, self.episode, ply, (self.game_offset + g) * 2 + side)
            cell, margin = boltzmann_expected(pi[g], self.temperature, u)
            self.samples += 1
            self.max_arg = max(self.max_arg, float(pi[g].max()) / float(np.float32(self.temperature)))
            self.nonuniform += len(np.unique(pi[g][pi[g] > 0])) > 1
            if margin < 1e-5:
                self.skipped += 1
            elif cell != int(actions[g]):
                self.mismatches.append((ply, g, int(actions[g]), cell, u))

    def finish(self, tag, min_samples, min_nonuniform=0):
        """min_nonuniform: how many samples must have come from a policy with unequal visit counts for the run to count as a test of that
        regime (while a root has untried actions every simulation expands one, and the policy is uniform over the visited cells: the move
        is then the same at every temperature)"""
        print(f"{tag}: T = {self.temperature}: {self.samples} samples ({self.nonuniform} from unequal visit counts, largest pi / T = {self.max_arg:.3f}), "
              f"{self.skipped} skipped (u within 1e-5 of a step), {len(self.mismatches)} mismatches")
        assert self.samples >= min_samples and self.nonuniform >= min_nonuniform
        assert not self.mismatches, f"{tag}: (ply, game, move, expected, u) = {self.mismatches[:5]}"
        assert self.skipped <= 0.02 * self.samples


def episode_records(n, total, sims, k, threshold, mode, seed, max_nodes, epsilon=0.25, alpha=0.03, temperature=1.0):
    """One whole episode of `total` games through SelfPlay.run: (packed replay records per game, status per game, stats)"""
    import torch
    import omok_ai_amd as oa
    eng = oa.Engine(board_size=n, games=total, max_nodes=max_nodes, max_tables=max_nodes // 2, max_batch_k=k, seed=seed, net_mode=mode)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    sp.reset()
    stats = sp.run(sims, k, epsilon, alpha, temperature, threshold)
    rec = sp.replay_record_bytes()
    _, _, plies = sp.game_info()
    _, status, _ = sp.game_info()
    lens = [len(sp.replay(g)[1]) for g in range(total)]
    buf = torch.zeros((sum(lens) + 1) * rec, dtype=torch.uint8, device="cuda")
    assert sp.replay_pack_into(buf.data_ptr(), sum(lens) + 1) == sum(lens)
    out = buf.cpu().numpy().reshape(-1, rec)
    offs = np.concatenate([[0], np.cumsum(lens)])
    games = [out[offs[g]:offs[g + 1]].copy() for g in range(total)]
    eng.close()
    return games, [int(s) for s in status], stats


def trained_tensors(n, seed, steps=200):
    """Weights after `steps` TrainPhase steps (Adadelta on the augmented replay records of a short self-play episode of the
    random-init net `seed`), on the GPU.  Returns (trained tensors, initial tensors)."""
    import torch
    import omok_ai_amd as oa
    from omok_ai_amd import train as T
    tensors = oa.weights.init_random(n, seed=seed)
    eng = oa.Engine(board_size=n, games=32, max_nodes=512, max_tables=256, max_batch_k=8, seed=4 + seed)
    eng.load_weights(tensors)
    sp = oa.SelfPlay(eng)
    sp.reset()
    sp.run(32, 8)
    _, _, plies = sp.game_info()
    rec = sp.replay_record_bytes()
    total = 6 * int(plies.sum())
    buf = torch.empty(total * rec, dtype=torch.uint8, device="cuda")
    assert sp.replay_augment_into(buf.data_ptr(), total) == total
    ph = T.TrainPhase(n, tensors, "cuda")
    ph.run(buf, update_count=steps, batch_size=128, seed=seed)
    trained = ph.net.tensors()
    eng.close()
    return trained, tensors


def _makes_a_line(cells, n):
    """True if the (at most five) cells are five in a row, column or diagonal -- the only way a side with five stones can end a game."""
    if len(cells) < 5:
        return False
    pts = sorted((c // n, c % n) for c in cells)
    dy, dx = pts[1][0] - pts[0][0], pts[1][1] - pts[0][1]
    return (dy, dx) in ((0, 1), (1, 0), (1, 1), (1, -1)) and all(
        (b[0] - a[0], b[1] - a[1]) == (dy, dx) for a, b in zip(pts, pts[1:]))


def scripted_finish(n, games, live, seed, winner="black", pattern="permuted"):
    """Per-ply moves for omok_play_actions that leave exactly `live` of `games` games alive: (actions [plies][games] int32, doomed [games] bool,
    status of a doomed game).  Doomed games play the five-in-a-row script of test_game_endings: Black 0..3 on row 0, White 0..3 on row 1, then
    winner == "black": Black completes row 0 with cell 4 on ply 9 (White is to move in the surviving games), winner == "white": Black plays a far
    cell, White completes row 1 on ply 10 (Black is to move).  Every doomed game ends on the LAST ply, so every game moves on every ply.  Surviving games
    play seeded random distinct cells, a different sequence per game; a sequence whose five stones of one colour would form a line is redrawn.  Which
    games are doomed: pattern == "permuted": a seeded permutation (runs of dead games of varying length) that always includes game 0 and the last game
    when at least two games are doomed; "alternate": every second game (live must be games // 2)."""
    assert n in (9, 15) and 0 <= live <= games and winner in ("black", "white")
    rng = np.random.default_rng([seed, n, games, live])
    hw, plies = n * n, 9 if winner == "black" else 10
    dead = games - live
    doomed = np.zeros(games, dtype=bool)
    if pattern == "alternate":
        assert live == games // 2
        doomed[1 - games % 2::2] = True  # (an odd game count: the even games, so that exactly games // 2 stay)
    else:
        assert pattern == "permuted"
        order = [int(g) for g in rng.permutation(games)]
        if dead >= 2:
            order = [0, games - 1] + [g for g in order if g not in (0, games - 1)]
        doomed[order[:dead]] = True
    assert int(doomed.sum()) == dead
    script = [0, n, 1, n + 1, 2, n + 2, 3, n + 3] + ([4] if winner == "black" else [5 * n + 7, n + 4])
    actions = np.zeros((plies, games), dtype=np.int32)
    for g in range(games):
        if doomed[g]:
            actions[:, g] = script
            continue
        while True:
            seq = rng.permutation(hw)[:plies]
            if not _makes_a_line(seq[0::2], n) and not _makes_a_line(seq[1::2], n):
                break
        actions[:, g] = seq
    return actions, doomed, 2 if winner == "black" else 3  # GameStatus::BlackWin / WhiteWin


def plan_text(plan):
    """one-line form of Engine.last_plan()"""
    t = f"{plan['path']} rows<={plan['rows']} nsplit {plan['nsplit']} tsplit {plan['tsplit']}"
    if plan["path"] in ("copy", "difference"):
        t += f" runs {plan['runs']} singles {plan['singles']} run-rows {plan['run_rows']}"
    if plan["path"] == "difference":
        t += f" full-runs {plan['full_runs']} tiles {plan['tiles']} t_split {plan['t_split']} ways {plan['ways']} fways {plan['fways']}"
    return t


def _ladder():
    """The points of tests/test_gpu_launch_shapes.py, picked from the output of tools/scan_launch_shapes.py on an MI355X (256 CUs) so that the plans
    they take cover the planner classes that test asserts; tests/test_launch_shape_scripts.py checks their scripts without a GPU."""
    pts = []

    def add(board, k, games, modes, lives, winner="black", pattern="permuted", cache=True):
        for live in lives:
            pts.append({"board": board, "k": k, "games": games, "modes": tuple(modes), "live": live, "winner": winner, "pattern": pattern, "cache": cache})

    # the headline engine: the tail of an episode of 4096 games (board 15, K = 16)
    add(15, 16, 4096, ["fp6"], [1, 9, 41, 100, 191, 192, 257, 513, 1025, 1850, 1950, 2300, 4096])
    add(15, 16, 4096, ["mixed"], [2, 127, 128, 512, 777, 1900, 2000, 3800], winner="white")
    add(15, 16, 4096, ["f16"], [24, 64, 191, 192])
    add(15, 16, 4096, ["f16"], [1024], cache=False)
    add(15, 16, 4096, ["f16"], [2048], winner="white", pattern="alternate", cache=False)
    add(15, 16, 4096, ["default"], [127, 128, 191, 192])
    # the same rows under a smaller partial slab
    add(15, 16, 1024, ["fp6", "f16"], [9, 100, 1024])
    add(15, 16, 192, ["fp6", "f16", "mixed"], [1, 191, 192])
    add(15, 16, 192, ["mixed"], [127, 128], winner="white")
    # board 9: hw % 32 = 17 (the partial pixel tile), 162 super-steps (the no-empty-split rule), 9 window bins
    add(9, 8, 2048, ["fp6"], [1, 16, 127, 128, 129, 300, 1000, 2048])
    add(9, 8, 2048, ["mixed"], [128, 1000, 2048], winner="white")
    add(9, 8, 2048, ["f16"], [127], winner="white")
    add(9, 8, 2048, ["f16"], [128], cache=False)
    add(9, 8, 2048, ["f16"], [1024], winner="white", pattern="alternate", cache=False)
    return pts


LAUNCH_SHAPE_LADDER = _ladder()

"""Shared helpers of the parity tests (no GPU, no product code)."""
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

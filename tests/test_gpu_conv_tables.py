"""k_sib_children2 takes conv_in's output and block 0's first layer from the conv tables (k_conv_tables: eight rows, one per 3-bit input pattern of a
pixel, rebuilt at every commit) instead of computing them in every pass.

  (1) every pattern through the kernel: rounds on the difference path from positions between near empty and more than half full, both sides to move, stones
      in corners and on edges.  Asserted from round_inputs(): all eight patterns occur among the pixels of the compared rows and each of the six stone patterns
      occurs at a P0 (the pixel a child differs from its base in: the only pixel that reads the second table).  Every row against an OMOK_NET_F32 engine,
      48 rows per round against the oracle, and against k_sib_children (omok_debug_set_children_kernel(1)) where the format has it.
  (2) the tables follow the weights: commit A, load + commit B, native train_step + commit -- after each the engine's rounds equal a fresh engine's, bit for bit.

The pixel of the net is a triple of the flat encoder.rs row (encoder.rs:10-46): pixel q = inputs 3 q .. 3 q + 2, input 2 c = the side to move's stone on cell c,
2 c + 1 = the other side's, inputs 2 HW .. = 1 if Black is to move; pattern = b0 | b1 << 1 | b2 << 2.  A cell cannot hold both colours, so a stone pixel shows
1..6 (3 only where the triple starts on an odd input, 6 only on an even one), and 7 / 0 come from the turn pixels.  positions.quiet gives the sparse positions
(it stops at 8 stones); the dense ones are random subsets of helpers.draw_sequence's colouring, whose lines hold runs of at most four."""
import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
from helpers import draw_sequence

TOL = 1e-3
# (n, games, k, rows from which a round takes the difference path, stone counts of the stages)
SHAPES = {15: (224, 16, 3072, (4, 7, 113, 150)), 9: (160, 8, 1024, (4, 7, 41, 60))}
ROUNDS = 3


def _dense(n, games, stones, seed):
    """boards [games][HW] of `stones` stones: random subsets of the five-free colouring of helpers.draw_sequence (a subset of runs <= 4 holds no five)"""
    seq = draw_sequence(n)
    black, white = np.array(seq[0::2]), np.array(seq[1::2])
    rng = np.random.default_rng([seed, n, games, stones])
    boards = np.zeros((games, n * n), dtype=np.uint8)
    for g in range(games):
        boards[g][rng.choice(black, (stones + 1) // 2, replace=False)] = O.BLACK
        boards[g][rng.choice(white, stones // 2, replace=False)] = O.WHITE
    return boards


def _stage_boards(n, games, stones):
    if stones > 8:
        return _dense(n, games, stones, 7)
    boards = P.quiet(n, games, stones, 7)
    if stones == 4:
        boards[0] = P.edge_positions(n)["corners"]  # a stone in every corner
    return boards


def _encode(n, boards, turn):
    """encoder.rs rows [G][3 HW] of boards with `turn` (0 = Black) to move, in numpy"""
    hw = n * n
    x = np.zeros((len(boards), 3 * hw), dtype=np.float32)
    mine, theirs = (O.BLACK, O.WHITE) if turn == 0 else (O.WHITE, O.BLACK)
    x[:, 0:2 * hw:2] = boards == mine
    x[:, 1:2 * hw:2] = boards == theirs
    x[:, 2 * hw:] = 1.0 if turn == 0 else 0.0
    return x


def _patterns(n, x):
    """pattern of every pixel of the rows x: [R][HW] ints"""
    t = (np.asarray(x).reshape(len(x), n * n, 3) > 0.5).astype(np.int64)
    return t[:, :, 0] | t[:, :, 1] << 1 | t[:, :, 2] << 2


def _p0_patterns(n, x, boards, stones):
    """patterns at P0 of the rows that are a stage position + ONE stone (children of a root; their base is the root's position seen by the other side): the
    new stone is the mover's, so it sits in input 2 c + 1 of the child's row, pixel (2 c + 1) // 3.  Rows that fit more than one game's position are left out."""
    hw = n * n
    occ = (x[:, 0:2 * hw:2] + x[:, 1:2 * hw:2] > 0.5).astype(np.float32)
    rows = np.flatnonzero(occ.sum(axis=1) == stones + 1)
    if not len(rows):
        return []
    fits = occ[rows] @ (boards != 0).astype(np.float32).T == stones  # [rows][games]
    pat, out = _patterns(n, x[rows]), []
    for i in np.flatnonzero(fits.sum(axis=1) == 1):
        g = int(np.argmax(fits[i]))
        c = int(np.flatnonzero(occ[rows[i]] - (boards[g] != 0) > 0.5)[0])
        assert x[rows[i], 2 * c + 1] == 1.0  # (the other side's stone, from the child's side to move)
        out.append(int(pat[i, (2 * c + 1) // 3]))
    return out


@pytest.mark.parametrize("n", [15, 9])
def test_stage_positions_can_show_every_pattern(n):
    """No GPU: the stage positions are legal, the numpy encoder above is the oracle's, and the children of the stage positions show all eight patterns among
    their pixels and all six stone patterns at P0 -- the GPU test asserts the same of the rows the search really asks for."""
    games, k, _, stages = SHAPES[n]
    seen, seen_p0, turns = set(), set(), set()
    for stones in stages:
        boards = _stage_boards(n, games, stones)
        assert all(int(np.count_nonzero(b)) == stones for b in boards)
        for b in boards[:6]:
            assert P.verdict(n, b) == (P.LEGAL, stones)
        turn = stones & 1
        turns.add(turn)
        assert np.array_equal(_encode(n, boards[:6], turn), P.input_rows(n, boards[:6]))
        for g in range(12):  # every child of the first positions
            empty = np.flatnonzero(boards[g] == 0)
            kids = np.repeat(boards[g][None], len(empty), axis=0)
            kids[np.arange(len(empty)), empty] = O.BLACK if turn == 0 else O.WHITE
            x = _encode(n, kids, turn ^ 1)
            seen |= set(np.unique(_patterns(n, x)).tolist())
            seen_p0 |= set(_p0_patterns(n, x, boards[g:g + 1], stones))
    e = n - 1
    assert boards.any(axis=0)[[0, e, e * n, e * n + e]].all() and _stage_boards(n, games, 4)[0][[0, e, e * n, e * n + e]].all()  # corners, dense and sparse
    assert turns == {0, 1} and seen == set(range(8)) and seen_p0 == {1, 2, 3, 4, 5, 6}, (seen, seen_p0)


def _play(eng, n, k, stages, games, want_logits):
    """per stage and round: (stones, x, p, v, logits, vpre, the round ran k_sib_children2)"""
    sp = oa.SelfPlay(eng)
    out = []
    for stones in stages:
        sp.reset_from(_stage_boards(n, games, stones))
        for rnd in range(ROUNDS):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            x = sp.round_inputs().copy()
            before = eng.stats()
            p, v = sp.round_eval()
            lg, vp = sp.round_logits() if want_logits else (None, None)
            after = eng.stats()
            sp.round_scatter()
            out.append((stones, x, np.array(p).reshape(nreq, -1).copy(), np.array(v).reshape(-1).copy(), lg, vp,
                        after["children2_launches"] - before["children2_launches"] == 1.0, after["children1_launches"] - before["children1_launches"] == 1.0))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [B.NET_F16X3_FP6, B.NET_F16X3_F16, B.NET_F16X3_MIXED])
@pytest.mark.parametrize("n", [15, 9])
def test_every_input_pattern_through_the_children_kernel(n, mode):
    """(1) of the module text.  Bounds: the project's 1e-3 contract against the fp32 kernels (p, v, logits, pre-tanh value) and the oracle (p, v); 2e-4 between
    the two children kernels as test_both_children_kernels_of_the_difference_path_agree asserts (the mixed format has k_sib_children2 only)."""
    games, k, diff_rows, stages = SHAPES[n]
    tensors = oa.weights.init_random(n, seed=4)
    eng = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=13, net_mode=mode)
    eng.load_weights(tensors)
    rounds = _play(eng, n, k, stages, games, True)
    eng.close()
    f32 = oa.Engine(board_size=n, games=games, max_nodes=64, max_tables=32, max_batch_k=k, seed=13, net_mode=B.NET_F32)
    f32.load_weights(tensors)
    net = O.Net(n, tensors)
    rng = np.random.default_rng(1)
    seen, seen_p0, compared, worst, worst_o = set(), set(), 0, np.zeros(4), np.zeros(2)
    for stones, x, p, v, lg, vp, ran2, _ in rounds:
        if not ran2:
            continue
        assert len(x) >= diff_rows
        compared += 1
        seen |= set(np.unique(_patterns(n, x)).tolist())
        seen_p0 |= set(_p0_patterns(n, x, _stage_boards(n, games, stones), stones))
        pf, vf = f32.evaluate_pv(x)
        lf, vpf = f32.evaluate_logits(x)
        d = [float(np.abs(a.reshape(len(x), -1) - b.reshape(len(x), -1)).max()) for a, b in ((p, pf), (v, vf), (lg, lf), (vp, vpf))]
        worst = np.maximum(worst, d)
        pick = rng.choice(len(x), size=48, replace=False)
        pc, vc = net.forward(x[pick], threads=8)
        worst_o = np.maximum(worst_o, [float(np.abs(p[pick] - pc).max()), float(np.abs(v[pick] - vc).max())])
    f32.close()
    print(f"n={n} mode {mode}: {compared} rounds on the difference path; against the fp32 kernels |dp| {worst[0]:.2e} |dv| {worst[1]:.2e} |dlogit| {worst[2]:.2e} "
          f"|dvpre| {worst[3]:.2e}; against the oracle |dp| {worst_o[0]:.2e} |dv| {worst_o[1]:.2e}; patterns {sorted(seen)}, at P0 {sorted(seen_p0)}")
    assert compared >= 2 * len(stages)
    assert seen == set(range(8)) and seen_p0 == {1, 2, 3, 4, 5, 6}, (seen, seen_p0)
    assert worst.max() < TOL and worst_o.max() < TOL, (worst, worst_o)
    if mode == B.NET_F16X3_MIXED:
        return
    one = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=13, net_mode=mode)
    one.load_weights(tensors)
    one.set_children_kernel(1)
    rounds1 = _play(one, n, k, stages, games, False)
    one.close()
    differing = pairs = 0
    for (_, xa, pa, va, _, _, ran2, _), (_, xb, pb, vb, _, _, _, ran1) in zip(rounds, rounds1):
        if not ran2:
            continue
        assert ran1 and np.array_equal(xa, xb)
        assert np.abs(pa - pb).max() < 2e-4 and np.abs(va - vb).max() < 2e-4, (float(np.abs(pa - pb).max()), float(np.abs(va - vb).max()))
        differing += int((pa.view(np.uint32) != pb.view(np.uint32)).any(axis=1).sum())
        pairs += len(xa)
    print(f"children kernels 2 vs 1, n={n} mode {mode}: {differing} of {pairs} rows differ in bits")


def _round_outputs(eng, n, games, k, rounds=2):
    sp = oa.SelfPlay(eng)
    sp.set_episode(0)  # (every reset moves on to the next RNG stream: a fresh engine's first reset uses stream 0)
    sp.reset_from(_stage_boards(n, games, SHAPES[n][3][2]))
    out = []
    for rnd in range(rounds):
        nreq = sp.round_generate(rnd, k, 0.25, 0.03)
        p, v = sp.round_eval()
        lg, vp = sp.round_logits()
        out.append((sp.round_inputs().copy(), np.array(p).reshape(nreq, -1).copy(), np.array(v).reshape(-1).copy(), lg.copy(), vp.copy()))
        sp.round_scatter()
    return out


def _same_rounds(a, b, tag):
    assert len(a) == len(b)
    for rnd, (ra, rb) in enumerate(zip(a, b)):
        for what, ta, tb in zip(("inputs", "p", "v", "logits", "vpre"), ra, rb):
            assert ta.shape == tb.shape and np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), f"{tag}: {what} of round {rnd} differ"


@pytest.mark.gpu
def test_tables_follow_the_weights():
    """(2) of the module text: an engine whose tables did not track a commit would evaluate block 0 of every child with the previous weights' conv_in.  After
    each of: commit of weights A, load + commit of weights B (another seed: every weight tensor different, conv_in's and block 0's among them), three native train_steps + commit --
    the engine's rounds on the difference path equal, bit for bit, those of a fresh engine loaded with read_weights()."""
    import torch
    n = 9  # (the tables and their rebuild do not depend on the board size: the small board keeps the test short)
    games, k, diff_rows, _ = SHAPES[n]

    def engine(tensors):
        e = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=13, net_mode=B.NET_F16X3_MIXED)  # (a set format: no probe at commit)
        e.load_weights(tensors)
        return e

    def against_fresh(eng, tag):
        eng.reset_stats()
        mine = _round_outputs(eng, n, games, k)
        assert eng.stats()["children2_launches"] == len(mine) and all(len(r[0]) >= diff_rows for r in mine)
        fresh = engine(eng.read_weights())
        _same_rounds(mine, _round_outputs(fresh, n, games, k), tag)
        fresh.close()
        return mine

    wa, wb = oa.weights.init_random(n, seed=4), oa.weights.init_random(n, seed=5)
    names = oa.weights.tensor_names()
    for name in ("conv_w", "residual_0_conv0_w"):  # conv_in and block 0's first layer (the random init leaves every bias zero)
        assert not np.array_equal(np.ravel(wa[names.index(name)]), np.ravel(wb[names.index(name)])), name
    eng = engine(wa)
    ra = against_fresh(eng, "weights A")
    eng.load_weights(wb)
    rb = against_fresh(eng, "weights B after A")
    assert not np.array_equal(ra[1][1], rb[1][1])
    # records for the training steps: a few plies of the engine's own self-play
    sp = oa.SelfPlay(eng)
    sp.reset()
    plies = 2
    sp.run(16, 8, max_plies=plies)
    rec, cap = sp.replay_record_bytes(), games * plies
    buf = torch.zeros(cap * rec, dtype=torch.uint8, device="cuda")
    got = sp.replay_pack_into(buf.data_ptr(), cap)
    assert got >= 128
    eng.train_begin(128)
    for step in range(3):
        eng.train_step(buf.data_ptr(), got, np.arange(128) + step)
    eng.commit()
    assert not np.array_equal(eng.read_weights()[0], np.ravel(wb[0]))  # (the steps moved conv_in)
    rc = against_fresh(eng, "after train_step + commit")
    assert not np.array_equal(rb[1][1], rc[1][1])
    eng.train_end()
    eng.close()

"""A/B of two builds of the library on the same inputs (bit-identity of kernel rewrites that must not change arithmetic): plain rows through
k_trunk (floats and board bits), and the pre-softmax logits of one search round on every sibling path -- the difference path with k_sib_children2 and
with k_sib_children, and the copy path -- in each operand format, at both board sizes.
usage: OMOK_MI355X_LIB=<lib.so> python tools/ab_net.py <out.npz> [n]   (run once per build, then compare the two files with
python tools/ab_net.py --compare a.npz b.npz)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    ok = True
    for k in a.files:
        same = np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
        print(k, "bit-identical" if same else f"DIFFERENT: max abs diff {np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max():.3e}")
        ok &= same
    sys.exit(0 if ok else 1)

import omok_ai_amd as oa
from omok_ai_amd import binding as B

# one search round per case: (tag, children kernel, games at N = 15 / 9, net modes); K = 16 at N = 15, 8 at N = 9.  224 x 16 = 3584 >= 3072 and
# 160 x 8 = 1280 >= 1024 rows take the difference path, 40 games stay on the copy path
ROUND_CASES = [("diff", 2, {15: 224, 9: 160}, {"fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16, "mixed": B.NET_F16X3_MIXED}),
               ("diffk1", 1, {15: 224, 9: 160}, {"fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16}),
               ("copy", 2, {15: 40, 9: 40}, {"fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16})]


def round_case(n, games, k, mode, which, want_path):
    """logits and pre-tanh values of the second search round from the start position (the first one whose requests are runs of siblings)"""
    eng = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=13, net_mode=mode)
    eng.load_random_weights(4)
    eng.set_children_kernel(which)
    sp = oa.SelfPlay(eng)
    sp.reset()
    for rnd in range(2):
        nreq = sp.round_generate(rnd, k, 0.25, 0.03)
        before = eng.stats()
        sp.round_eval()
        lg, vp = sp.round_logits()
        plan, st = eng.last_plan(), eng.stats()
        sp.round_scatter()
    assert plan["path"] == want_path and 0 < nreq <= games * k and plan["rows"] == games * k and plan["run_rows"] > 0, (n, games, k, mode, which, nreq, plan)
    if want_path == "difference":
        ran = tuple(st[c] > before[c] for c in ("children2_launches", "children1_launches"))  # launches of the recorded round alone
        assert ran == ((True, False) if which == 2 else (False, True)), (which, st)
    eng.close()
    return lg.copy(), vp.copy()


out = {}
for n in (9, 15):
    eng = oa.Engine(board_size=n, games=64, max_nodes=256, max_tables=64, max_batch_k=16, seed=1)
    eng.load_random_weights(0)
    rng = np.random.default_rng(0)
    hw = n * n
    x = np.zeros((700, 3 * hw), dtype=np.float32)
    for i in range(len(x)):  # encoder-layout rows of random positions
        k = int(rng.integers(0, hw))
        cells = rng.permutation(hw)[:k]
        turn = k % 2
        for j, c in enumerate(cells):
            mine = (j % 2) == turn
            x[i, 2 * c + (0 if mine else 1)] = 1.0
        x[i, 2 * hw:] = 1.0 if turn == 0 else 0.0
    p, v = eng.evaluate_pv(x)           # FROM_F32 path of the trunk
    lg, vp = eng.evaluate_logits(x)
    out[f"p{n}"], out[f"v{n}"], out[f"lg{n}"] = p, v, lg
    sp = oa.SelfPlay(eng)               # board-bits path of the trunk: a few plies of self-play, then the trees' statistics
    sp.reset()
    sp.run(32, 16, 0.25, 0.03, 1.0, 30, 6)
    out[f"w{n}"] = np.concatenate([sp.tree_dump(g, s)[1].reshape(-1) for g in range(8) for s in (0, 1)])
    eng.close()
    for tag, which, games, modes in ROUND_CASES:
        for mname, mode in modes.items():
            lg, vp = round_case(n, games[n], 16 if n == 15 else 8, mode, which, "copy" if tag == "copy" else "difference")
            out[f"{tag}_{mname}_lg{n}"], out[f"{tag}_{mname}_vp{n}"] = lg, vp
np.savez(sys.argv[1], **out)
print("saved", sys.argv[1])

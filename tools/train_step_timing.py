"""Cost of one training update: the engine's native step (omok_train_run) beside the torch autograd phase (train.TrainPhase.run).

Board 15, batches of 128 transitions (src/config.rs:83-110), records of a short self-play episode packed on the device by
omok_replay_augment_dev.  Each backend runs `--updates` updates (600 = parameter_update_count) as one blocking call; the figure is the median
of `--runs` such calls after `--warmup` discarded ones, divided by the update count.  A third leg runs the data-parallel backend's loop at world
size 1 (Trainer._train_data_parallel: omok_train_batch_indices, omok_train_backward into a slab, dist.gather_gradients, omok_train_apply of the
[1, count] slab), whose cost over omok_train_run is its host synchronisations per step.  Last, omok_train_apply's Adadelta launch alone under
HIP events (OMOK_STAT_MS_TRAIN_APPLY with omok_set_profiling) on synthetic slabs of 1, 2 and 8 ranks, beside the launch omok_train_step uses
(no slabs).  No threshold is attached: the figures go to profiles/ and DESIGN 8.
    python tools/train_step_timing.py [--updates 600] [--runs 5] [--warmup 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import omok_ai_amd as oa  # noqa: E402
from omok_ai_amd import train as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--games", type=int, default=16)
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = 15
    tensors = oa.weights.init_random(n, seed=0)
    eng = oa.Engine(board_size=n, games=a.games, max_nodes=1024, max_tables=512, max_batch_k=16, seed=7)
    eng.load_weights(tensors)
    sp = oa.SelfPlay(eng)
    sp.reset()
    sp.run(32, 16, 0.25, 0.03, 1.0, 30, a.plies)
    _, _, plies = sp.game_info()
    rec = sp.replay_record_bytes()
    total = 6 * int(plies.sum())
    buf = torch.zeros(total * rec, dtype=torch.uint8, device="cuda:0")
    assert sp.replay_augment_into(buf.data_ptr(), total) == total
    torch.cuda.synchronize()

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(i)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[a.warmup:]

    eng.train_begin(a.batch)
    native = timed(lambda i: eng.train_run(buf.data_ptr(), total, a.updates, a.batch, key=i))  # (includes its omok_net_commit)
    commit = timed(lambda i: eng.commit())

    count = eng.train_gradient_count()
    slab = torch.zeros(count, dtype=torch.float32, device="cuda:0")

    def dp_loop(key):  # trainer.Trainer._train_data_parallel at world size 1, without its commit
        for s in range(a.updates):
            idx = eng.train_batch_indices(total, a.batch, key, s)
            eng.train_backward(buf.data_ptr(), total, idx, slab.data_ptr())
            gathered = oa.dist.gather_gradients(slab)
            torch.cuda.current_stream().synchronize()
            eng.train_apply(gathered.data_ptr(), 1)

    dp = timed(dp_loop)
    eng.commit()

    # the rank-summing Adadelta launch alone: HIP events around it, synthetic slabs (the arithmetic does not depend on the values)
    slabs = torch.randn((8, count), dtype=torch.float32, device="cuda:0") * 1e-3
    torch.cuda.synchronize()
    eng.set_profiling(True)
    small = list(range(min(8, total)))
    kernel = {}
    for ranks in (0, 1, 2, 8):  # 0: no slabs, the launch of omok_train_step
        ms = []
        for _ in range(a.warmup + max(a.runs, 10)):
            eng.train_backward(buf.data_ptr(), total, small)
            before = eng.stats()["ms_train_apply"]
            if ranks == 0:
                eng.train_apply(None, 1)
            else:
                eng.train_apply(slabs.data_ptr(), ranks)
            ms.append(eng.stats()["ms_train_apply"] - before)
        kernel[ranks] = ms[a.warmup:]
    eng.set_profiling(False)
    eng.commit()
    phase = T.TrainPhase(n, tensors, "cuda:0")
    torch_ms = timed(lambda i: phase.run(buf.reshape(-1, rec), a.updates, a.batch, seed=i))
    push = timed(lambda i: phase.push_to(eng))
    med = statistics.median
    lines = [
        f"training update at N = {n}, batch {a.batch}, {total} records of a {a.games}-game, {a.plies}-ply episode; {a.updates} updates per call, "
        f"median of {a.runs} calls after {a.warmup} warm-up calls ({torch.cuda.get_device_name(0)})",
        f"native  omok_train_run            {med(native) / a.updates:9.3f} ms per update   ({med(native):10.1f} ms per call, its omok_net_commit included; "
        f"runs {', '.join(f'{v:.1f}' for v in native)})",
        f"        omok_net_commit alone     {med(commit):9.1f} ms per call",
        f"torch   TrainPhase.run            {med(torch_ms) / a.updates:9.3f} ms per update   ({med(torch_ms):10.1f} ms per call; "
        f"runs {', '.join(f'{v:.1f}' for v in torch_ms)})",
        f"        TrainPhase.push_to        {med(push):9.1f} ms per call (31 x omok_net_load + omok_net_commit)",
        f"native / torch per update: {(med(native) / med(torch_ms)):.2f}",
        f"native  hip_dp loop, world 1      {med(dp) / a.updates:9.3f} ms per update   ({med(dp):10.1f} ms per call, no commit; "
        f"runs {', '.join(f'{v:.1f}' for v in dp)})",
        f"        omok_train_run - commit   {(med(native) - med(commit)) / a.updates:9.3f} ms per update;  the loop's draw fetch, slab copy and two host "
        f"synchronisations per step cost {(med(dp) - med(native) + med(commit)) / a.updates:.3f} ms per update",
        f"Adadelta launch of omok_train_apply alone (HIP events, {count} elements = {4 * count / 1e6:.1f} MB per slab; median of {len(kernel[1])}):",
    ]
    for ranks in (0, 1, 2, 8):
        moved = 4 * count * (7 if ranks == 0 else ranks + 7)  # grad / slabs read, acc, accu, w read and written, grad written (not for ranks = 0: 7 = 1 + 6)
        m = med(kernel[ranks])
        what = "k_adadelta (no slabs)  " if ranks == 0 else f"k_adadelta_ranks, R = {ranks}"
        lines.append(f"        {what}   {m * 1e3:9.1f} us   {moved / 1e6:8.1f} MB moved   {moved / m / 1e6:8.1f} GB/s")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()

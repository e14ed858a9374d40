"""Worker of tests/test_gpu_train_dp.py (not a test): one rank of a 2-rank data-parallel training run of the REAL engine, both ranks on the
one GPU of the box, `gloo` for the exchange (RCCL needs one GPU per rank; dist.gather_gradients stages the slabs through the host).  Each
rank runs Trainer(train_backend="hip_dp") for two iterations on its own shard of the games and saves the engine's weights before and
after.  Usage: python -m torch.distributed.run --nproc-per-node 2 ... tests/train_dp_worker.py OUT_DIR"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch.distributed as dist
    os.environ["LOCAL_RANK"] = "0"  # both ranks share the box's one GPU
    from omok_ai_amd import trainer as TR
    out = sys.argv[1]
    dist.init_process_group("gloo")
    p = TR.Parameters(model_name="tiny", train_backend="hip_dp", episode_count=8, evaluate_count=16, evaluate_batch_size=8,
                      parameter_update_count=5, parameter_update_batch_size=32, evaluate_every=0)
    tr = TR.Trainer(p, board_size=9, seed=3, save_dir=os.path.join(out, "saves"), precision_rows=0)
    assert tr.world == 2 and tr.rank == dist.get_rank()
    before = tr.engine.read_weights()
    logs = []
    losses = tr.train(2, log=logs.append)
    after = tr.engine.read_weights()
    records = int(logs[-1].split("transitions=")[1].split()[0])
    np.savez(os.path.join(out, f"rank{tr.rank}.npz"), world=tr.world, rank=tr.rank, losses=np.asarray(losses, np.float64), records=records,
             **{f"w{i}": t for i, t in enumerate(after)}, **{f"i{i}": t for i, t in enumerate(before)})
    dist.barrier()
    dist.destroy_process_group()
    tr.close()


if __name__ == "__main__":
    main()

"""One fixed small scenario through every host driver of csrc/engine.cpp, and the comparison of two kernel traces of it.

  python tools/driver_scenario.py                      plays the scenario (9 x 9, 8 games, K = 8, 32 simulations) and prints a digest of its results
  python tools/driver_scenario.py --compare A.csv B.csv [--out FILE]
                                                       the ordered lists of (kernel name, grid, workgroup size) of two rocprofv3 kernel traces

A refactor of the host code must leave the launch sequence alone: run the scenario once per build of the library under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/driver_scenario.py` (no counters in the same pass; OMOK_MI355X_LIB selects
the other build) and compare the two *_kernel_trace.csv files.  The scenario: a self-play episode (run), step-wise plies in self-play and in a match,
four match plies (run), episodes from given positions (self-play and match), a versus episode, 24 games on 8 slots with the log, both shared-tree
executors with 4 waves."""
import csv
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, GAMES, K, COUNT = 9, 8, 8, 32


def _stepwise_ply(sp):
    for rnd in range(COUNT // K):
        sp.round_generate(rnd, K)
        sp.round_eval()
        sp.round_scatter()
    sp.sample_actions(1.0, 4)
    sp.mirror_generate()
    sp.mirror_eval()
    sp.mirror_apply()
    sp.execute(COUNT, K)
    sp.sample_actions(1.0, 4)
    sp.advance()


def scenario():
    import numpy as np
    import torch
    import omok_ai_amd as oa
    from omok_ai_amd import binding as B
    from omok_ai_amd import records as R

    h = hashlib.sha256()

    def note(tag, sp, eng):
        alive, status, plies = sp.game_info()
        st = eng.stats()
        h.update(alive.tobytes() + status.tobytes() + plies.tobytes())
        for g in range(eng.games):
            for side in (0, 1):
                ints, floats = sp.tree_dump(g, side)
                h.update(ints.tobytes() + floats.tobytes())
        print(f"{tag}: ply {sp.ply} alive {int(alive.sum())} plies {int(plies.sum())} sims {int(st['sims'])} evals {int(st['evals'])} "
              f"ply_games {int(st['ply_games'])} finished {int(st['finished'])} sha256 {h.hexdigest()[:16]}", flush=True)

    eng = oa.Engine(board_size=N, games=GAMES, max_nodes=1024, max_tables=512, max_batch_k=K, seed=21)
    eng.load_random_weights(0)
    eng.load_weights2(oa.weights.init_random(N, seed=1))
    sp = oa.SelfPlay(eng)
    sp.reset()
    sp.run(COUNT, K, threshold=4)
    note("self-play episode", sp, eng)
    sp.reset()
    _stepwise_ply(sp)
    note("self-play, step-wise", sp, eng)
    sp.match_reset(GAMES // 2)
    sp.run(COUNT, K, threshold=4, max_plies=4)
    note("match, 4 plies", sp, eng)
    _stepwise_ply(sp)
    note("match, step-wise", sp, eng)
    boards, ok = eng.env_random_positions(5, 0, 4, GAMES)
    assert ok.all()
    sp.reset_from(boards)
    sp.run(COUNT, K, threshold=4, max_plies=2)
    note("self-play from positions", sp, eng)
    sp.match_reset_from(GAMES // 2, boards)
    sp.run(COUNT, K, threshold=4, max_plies=2)
    note("match from positions", sp, eng)
    sp.reset()
    res, _ = sp.versus_run(B.OPP_NAIVE, 0, COUNT, K)
    note(f"versus episode {res}", sp, eng)
    total, cap = 3 * GAMES, 3 * GAMES * N * N
    rec = torch.zeros(cap * sp.replay_record_bytes(), dtype=torch.uint8, device="cuda")
    log = torch.zeros(cap * R.ENTRY_BYTES, dtype=torch.uint8, device="cuda")
    sp.game_log(True)
    sp.reset()
    _, n_records, off, ln, stt = sp.run_slots_logged(total, COUNT, K, rec.data_ptr(), cap, log.data_ptr(), threshold=4)
    h.update(rec.cpu().numpy().tobytes() + log.cpu().numpy().tobytes() + off.tobytes() + ln.tobytes() + stt.tobytes())
    note(f"slots, logged: {n_records} records of {total} games", sp, eng)
    eng.close()

    eng = oa.Engine(board_size=N, games=1, max_nodes=1024, max_tables=512, max_batch_k=K, seed=21, max_tree_waves=4)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    sp.reset()
    sp.execute_shared(COUNT, K, waves=4)  # (the waves' lock order is not fixed from run to run: no digest of this tree)
    groups = sp.execute_shared_recorded(COUNT, K, waves=4)
    print(f"execute_shared + execute_shared_recorded, 4 waves: sims {int(eng.stats()['sims'])}, recorded groups (simulations, backups, requests)",
          [(len(so), len(bo), len(v)) for so, bo, _, v in groups])
    eng.close()


def _launches(path):
    rows = list(csv.DictReader(open(path)))
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    dims = [c for c in (rows[0] if rows else {}) if c.startswith("Grid_Size") or c.startswith("Workgroup_Size")]
    assert not rows or len(dims) == 6, f"{path}: grid / workgroup columns not found in {list(rows[0])}"
    return [(r["Kernel_Name"],) + tuple(int(r[c]) for c in sorted(dims)) for r in rows]


def compare(path_a, path_b, out):
    a, b = _launches(path_a), _launches(path_b)
    lines = [f"kernel traces of tools/driver_scenario.py: {os.path.basename(path_a)} ({len(a)} launches) against {os.path.basename(path_b)} ({len(b)} launches)",
             f"distinct kernels: {len(set(x[0] for x in a))} / {len(set(x[0] for x in b))}"]
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) == len(b):
        lines.append("the ordered lists of (kernel name, grid, workgroup size) are EQUAL")
    else:
        i = min(len(a), len(b)) if first is None else first
        lines.append(f"the lists DIFFER from launch {i} on:")
        for j in range(max(0, i - 2), i + 3):
            lines.append(f"  {j}: {a[j] if j < len(a) else None}\n     {b[j] if j < len(b) else None}")
    text = "\n".join(lines)
    print(text)
    if out:
        open(out, "w").write(text + "\n")
    return 0 if first is None and len(a) == len(b) else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == "--out" else None))
    scenario()

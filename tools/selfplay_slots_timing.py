"""What training on slots-mode self-play costs and gains (`python tools/selfplay_slots_timing.py [OUT.txt] [--games G] [--slots S] [--sims S] [--board N]`):
on one engine configuration (configs[1] by default: 4096 games, 15 x 15, 800 simulations, K = 16) games/s of an episode of `--games` games
(omok_selfplay_run on an engine of that many games) beside the same number of games on `--slots` slots (omok_selfplay_run_slots, default games / 4),
alternating -- 1 warm-up pair, then 3 pairs, medians -- then the post-processing of the slots run's raw records by
omok_replay_augment_records_dev beside omok_replay_augment_dev on the episode engine's games: the kernels under the engine's HIP events
(OMOK_STAT_MS_PLY with omok_set_profiling) and the wall clock of the blocking call, 3 warm-up calls, then 5, medians.  Both calls move about 7 records
per transition (one read, six written).
`--log` measures the move log in slots mode instead: on one engine of `--slots` slots, `--games` games with the log off (omok_selfplay_run_slots)
and on (omok_selfplay_run_slots_logged), alternating, the same warm-up and pairs, games/s; then the device-to-host read-back of the packed
log and records.GameRecords.from_packed of all games (SelfPlay.slots_game_records), wall clock, 1 warm-up call, then 5, median."""
import os
import sys
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omok_ai_amd as oa


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


games, sims, n = opt("--games", 4096), opt("--sims", 800), opt("--board", 15)
slots = opt("--slots", max(1, games // 4))
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
k = 16 if n == 15 else 8
max_nodes = min(16384, 4 * sims + 1024)
out = []


def say(line):
    print(line, flush=True)
    out.append(line)


def engine(g):
    eng = oa.Engine(board_size=n, games=g, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4), max_batch_k=k, seed=1)
    eng.load_random_weights(0)
    return eng, oa.SelfPlay(eng)


def log_leg():
    eng, sp = engine(slots)
    rec, cap = sp.replay_record_bytes(), games * n * n
    raw = torch.empty(cap * rec, dtype=torch.uint8, device="cuda")
    log = torch.empty(cap * oa.records.ENTRY_BYTES, dtype=torch.uint8, device="cuda")

    def run(logged):
        sp.game_log(logged)  # (allocates / frees the per-slot log outside the timed part; it starts at the reset)
        sp.reset()
        eng.reset_stats()
        t = time.perf_counter()
        if logged:
            res = sp.run_slots_logged(games, sims, k, raw.data_ptr(), cap, log.data_ptr())
        else:
            res = sp.run_slots(games, sims, k, raw.data_ptr(), cap)
        return res[0]["finished"] / (time.perf_counter() - t), res

    say(f"{games} games, {n} x {n}, {sims} simulations, K = {k}, slots mode on {slots} slots of one engine: move log off (omok_selfplay_run_slots) / on "
        "(omok_selfplay_run_slots_logged), alternating; 1 warm-up pair, then 3 pairs")
    run(False)
    run(True)
    rate = {"off": [], "on": []}
    for pair in range(3):
        rate["off"].append(run(False)[0])
        r, (_, n_raw, off, ln, status) = run(True)
        rate["on"].append(r)
        say(f"pair {pair}: log off {rate['off'][-1]:.2f} games/s, log on {r:.2f} games/s")
    for name in ("off", "on"):
        say(f"log {name}: median {np.median(rate[name]):.2f} games/s (min {min(rate[name]):.2f}, max {max(rate[name]):.2f})")
    say(f"log on / log off, medians: {np.median(rate['on']) / np.median(rate['off']):.4f}")
    wall = []
    for _ in range(6):
        t = time.perf_counter()
        games_rec = sp.slots_game_records(log, n_raw, off, ln, status)
        wall.append((time.perf_counter() - t) * 1e3)
    say(f"read-back of the packed log + GameRecords.from_packed, all {games_rec.games} games ({n_raw} moves, {n_raw * oa.records.ENTRY_BYTES / 1e6:.1f} MB): wall clock median "
        f"{np.median(wall[1:]):.3f} ms (min {min(wall[1:]):.3f}, max {max(wall[1:]):.3f})")
    eng.close()


if "--log" in sys.argv:
    log_leg()
    if args:
        open(args[0], "w").write("\n".join(out) + "\n")
    raise SystemExit(0)

e_eng, e_sp = engine(games)
s_eng, s_sp = engine(slots)
rec = e_sp.replay_record_bytes()
cap = games * n * n
raw = torch.empty(cap * rec, dtype=torch.uint8, device="cuda")


def episode():
    e_sp.reset()
    e_eng.reset_stats()  # (OMOK_STAT_FINISHED counts from here)
    t = time.perf_counter()
    st = e_sp.run(sims, k)
    return st["finished"] / (time.perf_counter() - t)


def slots_run():
    s_sp.reset()
    s_eng.reset_stats()
    t = time.perf_counter()
    st, n_raw, off, ln, _ = s_sp.run_slots(games, sims, k, raw.data_ptr(), cap)
    return st["finished"] / (time.perf_counter() - t), n_raw, off, ln


say(f"{games} games, {n} x {n}, {sims} simulations, K = {k}: an episode on {games} games' trees / slots mode on {slots} slots, alternating; 1 warm-up pair, then 3 pairs")
episode()
slots_run()
rate = {"episode": [], "slots": []}
for pair in range(3):
    rate["episode"].append(episode())
    r, n_raw, off, ln = slots_run()
    rate["slots"].append(r)
    say(f"pair {pair}: episode {rate['episode'][-1]:.2f} games/s, slots {r:.2f} games/s")
for name in ("episode", "slots"):
    say(f"{name}: median {np.median(rate[name]):.2f} games/s (min {min(rate[name]):.2f}, max {max(rate[name]):.2f})")
say(f"slots / episode, medians: {np.median(rate['slots']) / np.median(rate['episode']):.4f}")

# post-processing: the episode engine still holds its last episode; the slots run left its raw records in `raw`
_, _, plies = e_sp.game_info()
e_total, s_total = 6 * int(plies.sum()), 6 * int(ln.sum())
dst = torch.empty(max(e_total, s_total) * rec, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()


def timed(eng, call, want):
    eng.set_profiling(1)
    wall, ev = [], []
    for _ in range(8):
        eng.reset_stats()
        t = time.perf_counter()
        assert call() == want
        wall.append((time.perf_counter() - t) * 1e3)
        ev.append(eng.stats()["ms_ply"])
    eng.set_profiling(0)
    return np.median(wall[3:]), np.median(ev[3:]), min(ev[3:]), max(ev[3:])


ew, ek, ek0, ek1 = timed(e_eng, lambda: e_sp.replay_augment_into(dst.data_ptr(), e_total), e_total)
sw, sk, sk0, sk1 = timed(s_eng, lambda: s_eng.replay_augment_records(raw.data_ptr(), n_raw, off, ln, dst.data_ptr(), s_total), s_total)
say(f"omok_replay_augment_dev, {e_total // 6} transitions of {games} resident games ({7 * (e_total // 6) * rec / 1e6:.1f} MB moved): kernels under HIP events median "
    f"{ek:.3f} ms (min {ek0:.3f}, max {ek1:.3f}); wall clock of the blocking call median {ew:.3f} ms")
say(f"omok_replay_augment_records_dev, {s_total // 6} transitions of {games} games in completion order ({7 * (s_total // 6) * rec / 1e6:.1f} MB moved): kernel under HIP events median "
    f"{sk:.3f} ms (min {sk0:.3f}, max {sk1:.3f}); wall clock of the blocking call (host table, upload, kernel) median {sw:.3f} ms")
if e_total and s_total:
    say(f"per transition, records / resident: kernels {(sk / s_total) / (ek / e_total):.3f}, blocking call {(sw / s_total) / (ew / e_total):.3f}")
if args:
    open(args[0], "w").write("\n".join(out) + "\n")
e_eng.close()
s_eng.close()

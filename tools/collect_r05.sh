#!/bin/bash
# Round-5 evidence on the GPU box (run from the repo root): tools/collect_r05.sh gpurun_out/r05 [part...]   parts: tests bench pmc c3 misc (default: all)
out=${1:-gpurun_out/r05}; shift; parts=${@:-tests bench pmc c3 misc driver}; mkdir -p $out; R=$PWD
has() { [[ " $parts " == *" $1 "* ]]; }
if has tests; then
  echo "[tests]"; python -m pytest tests -q -m gpu -s > $out/gputests_full.log 2>&1; tail -2 $out/gputests_full.log
fi
if has bench; then
  echo "[bench c2, 3 steps]"; python3 bench.py --full --steps 3 --warmup 1 > $out/bench_c2_full_episode.json 2> $out/bench_c2.err; tail -c 200 $out/bench_c2_full_episode.json; echo
  echo "[kernel stats c2]"; tools/kstats.sh $out c2 --max-plies 4 | head -24
  cp $out/ks_c2.log $out/bench_c2_first4plies_under_rocprofv3.log 2>/dev/null
fi
if has pmc; then
  echo "[pmc c2]"; tools/collect_pmc.sh $out 15 | tail -14
fi
if has c3; then
  echo "[bench c3]"; python3 bench.py --full --board 9 --games 16384 --sims 200 --batch-k 8 --steps 2 --warmup 1 > $out/bench_c3_9x9_16384games.json 2> $out/bench_c3.err; tail -c 200 $out/bench_c3_9x9_16384games.json; echo
  tools/kstats.sh $out c3 --board 9 --games 16384 --sims 200 --batch-k 8 --max-plies 4 | head -16
  echo "[pmc c3]"; tools/collect_pmc.sh $out 9 --board 9 --games 16384 --sims 200 --batch-k 8 | tail -8
fi
if has misc; then
  echo "[bench c1]"; python3 bench.py --full --games 1 --sims 100 --batch-k 16 --cpu-seconds 0 > $out/bench_c1_single_game.json 2>/dev/null; tail -c 150 $out/bench_c1_single_game.json; echo
  echo "[rehearsal]"; OMOK_BENCH_BACKEND=gloo python bench.py --full --gpus 2 --games 256 --sims 64 --max-plies 6 --gather --cpu-seconds 0 > $out/rehearsal_2ranks_one_gpu_gloo.json 2> $out/rehearsal.err; tail -c 200 $out/rehearsal_2ranks_one_gpu_gloo.json; echo
  echo "[soak]"; (python tools/soak_determinism.py 1024 512 2 15 16 auto; python tools/soak_determinism.py 2048 200 2 9 8 auto) > $out/soak_determinism.log 2>&1; tail -3 $out/soak_determinism.log
  echo "[ply times]"; python tools/ply_times.py > $out/ply_times_by_live_games.txt 2>&1; tail -12 $out/ply_times_by_live_games.txt
fi
if has driver; then
  echo "[driver-style bench: --gpus 1 --steps 20 --warmup 5 --full]"; python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $out/bench_c2_20steps_driver_style.json 2> $out/bench_driver.err; head -c 300 $out/bench_c2_20steps_driver_style.json; echo
fi

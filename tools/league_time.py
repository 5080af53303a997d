"""Time the league step against the single-opponent wrapper (one process, alternating repetitions, medians).

    PYTHONPATH=. python tools/league_time.py [--envs 65536] [--steps 200] [--reps 7] [--out FILE.json]

A  TournamentEnvWrapper.step_device vs MEDIUM (the `tournament` workload's loop; this wrapper and its kernel launch are the ones
   of the commit before the league)
B  LeagueEnvWrapper.step_device, every env on MEDIUM
C  the league with a uniform per-env mix of RANDOM / WEAK / MEDIUM / RULE_BASED
D  RANDOM for every env: the league (actions drawn on the device) against the wrapper's host path (numpy + a copy per step)
Each repetition is `steps` steps between two events; the four pairs alternate A B A B ... so that clock drift hits both alike.
For the per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python tools/league_time.py --only C` (a run of its own).
"""
import argparse
import json
import statistics
import time

import torch

import competitive_rl_amd as crl
from competitive_rl_amd.league import LeagueEnvWrapper

NAMES = ["RANDOM", "WEAK", "MEDIUM", "RULE_BASED"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.envs

    def env():
        return crl.make_envs("cPongDouble-v0", num_envs=n, log_dir=None, seed=1, resized_dim=42, frame_stack=None)

    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.randint(0, 3, (args.steps, n), generator=g, device="cuda", dtype=torch.int32)
    runs = {}

    def add(key, wrapper, prepare):
        if args.only and key[0] not in args.only:
            return
        wrapper.reset()
        prepare(wrapper)
        runs[key] = wrapper

    add("A tournament MEDIUM", crl.TournamentEnvWrapper(env(), n), lambda w: w.reset_opponent("MEDIUM"))
    add("B league all MEDIUM", LeagueEnvWrapper(env(), n, NAMES), lambda w: w.set_opponents("MEDIUM"))
    add("C league uniform mix", LeagueEnvWrapper(env(), n, NAMES, seed=3), lambda w: w.reset_opponent())
    add("D0 tournament RANDOM (host)", crl.TournamentEnvWrapper(env(), n), lambda w: w.reset_opponent("RANDOM"))
    add("D1 league all RANDOM", LeagueEnvWrapper(env(), n, NAMES), lambda w: w.set_opponents("RANDOM"))

    def rep(w):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for t in range(args.steps):
            w.step_device(acts[t])
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps, (time.perf_counter() - t0) * 1e3 / args.steps

    for w in runs.values():  # warm-up
        rep(w)
    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, w in runs.items():
            ms[k].append(rep(w))
    res = {"envs": n, "steps_per_rep": args.steps, "reps": args.reps, "device": torch.cuda.get_device_name(0), "runs": {}}
    for k, v in ms.items():
        dev, wall = [x[0] for x in v], [x[1] for x in v]
        res["runs"][k] = {"device_ms_per_step_median": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
                          "wall_ms_per_step_median": statistics.median(wall), "all_device_ms": dev}
        print(f"{k:32s} {statistics.median(dev) * 1e3:9.1f} us/step device (min {min(dev) * 1e3:.1f}, max {max(dev) * 1e3:.1f}), "
              f"{statistics.median(wall) * 1e3:9.1f} us/step wall, {n / statistics.median(wall) / 1e3:.2f} M env-steps/s")
    if "C league uniform mix" in runs:
        res["C_counts"] = dict(zip(NAMES, runs["C league uniform mix"].counts().tolist()))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for w in runs.values():
        w.close()


if __name__ == "__main__":
    main()

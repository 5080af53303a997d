"""What serving the built-in CarRacing drivers costs (include/crl.h "car drivers"): ``CarDrivers.act`` + ``step_device`` against
``step_device`` alone, in ONE process on one env batch, the legs alternating inside every repeat.

    python tools/ab/car_drivers.py [--envs 16384] [--steps 200] [--repeats 7] [--warmup 1000] [--out FILE.json]

Both cars of every env are assigned (car 0 the default RULE_BASED style, car 1 RULE_BASED with epsilon 0.1).  Steady state as
bench.py makes it for the car workload: gym's TimeLimit counters staggered uniformly over [0, 1000), then `warmup` steps driven by the
drivers, un-timed -- the batch holds cars of every age, spread over their tracks, and every step carries its ~ envs / 1000 resets.  Then
every repeat times
  step        `steps` x step_device with the actions of the last act call (nothing else on the stream)
  act_step    `steps` x (act, step_device)
  act         `steps` x act alone
between two device events; one figure (ms per step) per leg and repeat.  Printed: each leg's repeats, median and spread
(max - min) / median, and act_step / step.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import competitive_rl_amd as crl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("car_drivers.py measures on the GPU; none is visible")
    n = args.envs
    env = crl.HipCarVecEnv(n, seed=0)
    drivers = crl.CarDrivers(env, seed=1)
    drivers.set_style("eps", epsilon=0.1)
    drivers.assign(0, "RULE_BASED"), drivers.assign(1, "eps")
    acts = torch.zeros((n, 2, 2), device="cuda")
    env.reset()
    st = env.get_state()
    st["elapsed"] = (np.arange(n, dtype=np.int64) * 1000 // n).astype(st["elapsed"].dtype)
    env.set_state(st)
    ended = torch.zeros((), dtype=torch.int64, device="cuda")

    def step():
        return env.step_device(acts)

    def act_step():
        drivers.act(acts)
        return env.step_device(acts)

    legs = {"step": step, "act_step": act_step, "act": lambda: drivers.act(acts)}
    for _ in range(args.warmup):
        ended += act_step()[2].sum()
    torch.cuda.synchronize()
    print("warmed up: %d steps, %d episodes ended" % (args.warmup, int(ended)), flush=True)
    order = list(legs)
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:  # (another leg goes first in every repeat)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                legs[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in order:
        print("%-10s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])), flush=True)
    st = env.get_state()
    out = {"envs": n, "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "ms": ms, "median_ms": med, "spread": spread,
           "act_step_over_step": med["act_step"] / med["step"], "mean_tiles_visited": float(st["car"]["tile_visited_count"].mean()),
           "cars_done": int(st["car"]["done"].sum())}
    print("act_step / step = %.4f (%+.4f ms); act alone %.4f ms" % (out["act_step_over_step"], med["act_step"] - med["step"], med["act"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    drivers.close(), env.close()


if __name__ == "__main__":
    main()

"""What serving learned CarRacing drivers costs (include/crl.h "car policy"): ``CarPolicy.act_rollout`` against ``CarDrivers.act`` and
against the step it feeds, in ONE process on one env batch, the legs alternating inside every repeat.

    python tools/ab/car_policy.py [--envs 16384] [--steps 200] [--repeats 7] [--warmup 1000] [--weights FILE.npz] [--out FILE.json]

Both cars of every env are served by one sampling network (the worst case: every car runs the network and the draw): the weights of
``--weights`` (default tests/golden/car_policy_clone.npz, the net cloned from RULE_BASED) with log_std -2.  Steady state as
tools/ab/car_drivers.py makes it: gym's TimeLimit counters staggered uniformly over [0, 1000), then `warmup` steps driven by the policy,
un-timed.  Then every repeat times
  step          `steps` x step_device with the actions of the last act call (nothing else on the stream)
  policy_step   `steps` x (act_rollout, step_device)
  policy        `steps` x act_rollout alone (values, log-probs and the observation written)
  act           `steps` x act alone (actions only)
  observe       `steps` x observe alone: the search and the features without the network
  drivers       `steps` x CarDrivers.act alone (both cars RULE_BASED, car 1 with epsilon 0.1)
between two device events; one figure (ms per step) per leg and repeat.  Printed: each leg's repeats, median and spread
(max - min) / median, policy_step / step and policy / step.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import competitive_rl_amd as crl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "car_policy_clone.npz"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("car_policy.py measures on the GPU; none is visible")
    n = args.envs
    env = crl.HipCarVecEnv(n, seed=0)
    weights = dict(crl.rules.car_policy_weights(args.weights), log_std=np.full(2, -2.0, np.float32))
    policy = crl.CarPolicy(env, seed=1)
    policy.add_network("net", weights)
    policy.assign(0, "net"), policy.assign(1, "net")
    drivers = crl.CarDrivers(env, seed=1)
    drivers.set_style("eps", epsilon=0.1)
    drivers.assign(0, "RULE_BASED"), drivers.assign(1, "eps")
    acts = torch.zeros((n, 2, 2), device="cuda")
    spare = torch.zeros((n, 2, 2), device="cuda")  # what the drivers' leg writes: the step's actions stay the policy's
    obs = torch.zeros((n, 2, 21), device="cuda")
    env.reset()
    st = env.get_state()
    st["elapsed"] = (np.arange(n, dtype=np.int64) * 1000 // n).astype(st["elapsed"].dtype)
    env.set_state(st)
    ended = torch.zeros((), dtype=torch.int64, device="cuda")

    def policy_step():
        policy.act_rollout(acts, obs_out=obs)
        return env.step_device(acts)

    legs = {"step": lambda: env.step_device(acts), "policy_step": policy_step, "policy": lambda: policy.act_rollout(acts, obs_out=obs),
            "act": lambda: policy.act(acts), "observe": lambda: policy.observe(obs), "drivers": lambda: drivers.act(spare)}
    for _ in range(args.warmup):
        ended += policy_step()[2].sum()
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
        print("%-12s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])), flush=True)
    st = env.get_state()
    out = {"envs": n, "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "ms": ms, "median_ms": med, "spread": spread,
           "policy_step_over_step": med["policy_step"] / med["step"], "policy_over_step": med["policy"] / med["step"],
           "mean_tiles_visited": float(st["car"]["tile_visited_count"].mean()), "cars_done": int(st["car"]["done"].sum())}
    print("policy_step / step = %.4f (%+.4f ms); act_rollout alone %.4f ms = %.2f %% of the step; observe %.4f ms; CarDrivers.act %.4f ms" % (
        out["policy_step_over_step"], med["policy_step"] - med["step"], med["policy"], 100 * out["policy_over_step"], med["observe"], med["drivers"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    drivers.close(), policy.close(), env.close()


if __name__ == "__main__":
    main()

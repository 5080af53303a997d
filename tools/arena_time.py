"""Time the arena step with and without its books (one process, alternating repetitions, medians).

    PYTHONPATH=. python tools/arena_time.py [--envs 65536] [--steps 200] [--reps 7] [--out FILE.json]

a  LeagueArena.step_device over RANDOM / RULE_BASED / WEAK / MEDIUM with the pairs it starts with (every off-diagonal pair on the same
   number of envs) and NO books: crl_arena_step and crl_league_set_assignment skipped -- both bats served, the env stepped
b  the same arena as it ships: per step crl_arena_step (books + redraws, unit weights, so the mix stays uniform) and
   crl_league_set_assignment of the 2N virtual envs (a copy + the partition)
c  for scale: LeagueEnvWrapper(ledger=True, resample_on_done=True) on the same pool -- ONE seat served, the other bat's actions given
Each repetition is `steps` steps between two events; the runs alternate a b c a b c ... so that clock drift hits all alike.  `a` and `b`
run the CNN agents on twice as many frames as `c` by design.
For the per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python tools/arena_time.py --only b` (a run of its own).
"""
import argparse
import json
import statistics
import time

import torch

import competitive_rl_amd as crl
from competitive_rl_amd.arena import LeagueArena
from competitive_rl_amd.league import LeagueEnvWrapper

NAMES = ["RANDOM", "RULE_BASED", "WEAK", "MEDIUM"]


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

    def arena(books):
        w = LeagueArena(env(), n, NAMES, seed=3)
        if not books:
            w._after_step = lambda rew, done: None
        w.reset()
        return w

    def league():
        w = LeagueEnvWrapper(env(), n, NAMES, seed=3, resample_on_done=True, ledger=True)
        w.reset()
        w.reset_opponent()
        return w

    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.randint(0, 3, (args.steps, n), generator=g, device="cuda", dtype=torch.int32)
    runs = {}
    for key, make in (("a arena, fixed pairs, no books", lambda: arena(False)), ("b arena, books and redraws", lambda: arena(True)),
                      ("c league + ledger, one seat", league)):
        if not args.only or key[0] in args.only:
            runs[key] = make()

    def rep(w):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        one_seat = isinstance(w, LeagueEnvWrapper)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for t in range(args.steps):
            if one_seat:
                w.step_device(acts[t])
            else:
                w.step_device()
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
        print(f"{k:40s} {statistics.median(dev) * 1e3:9.1f} us/step device (min {min(dev) * 1e3:.1f}, max {max(dev) * 1e3:.1f}), "
              f"{statistics.median(wall) * 1e3:9.1f} us/step wall, {n / statistics.median(wall) / 1e3:.2f} M env-steps/s")
    med = {k[0]: r["device_ms_per_step_median"] for k, r in res["runs"].items()}
    if "a" in med and "b" in med:
        res["b_over_a"] = med["b"] / med["a"]
        print(f"b / a = {res['b_over_a']:.4f}")
    if "a" in med and "c" in med:
        res["a_over_c"] = med["a"] / med["c"]
        print(f"a / c = {res['a_over_c']:.4f}  (a serves two seats, c one)")
    for k, w in runs.items():
        if isinstance(w, LeagueArena):
            res["runs"][k]["episodes"] = w.counters()["episodes"].tolist()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for w in runs.values():
        w.close()


if __name__ == "__main__":
    main()

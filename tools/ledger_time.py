"""Time the league step with and without the results ledger (one process, alternating repetitions, medians).

    PYTHONPATH=. python tools/ledger_time.py [--envs 65536] [--steps 200] [--reps 7] [--out FILE.json]

a  LeagueEnvWrapper.step_device, uniform mix of RANDOM / WEAK / MEDIUM / RULE_BASED, resample_on_done=True (uniform redraws by
   crl_league_resample: the launches of the commit before the ledger)
b  the same league with ledger=True: per step a copy of the assignment, the ledger's launch (books + weighted redraws, unit weights, so
   the mix stays uniform) and crl_league_set_assignment (a copy + the partition that `a` runs inside crl_league_resample)
c  b with a pfsp_weights() call every 10 steps (the table then follows the books)
Each repetition is `steps` steps between two events; the runs alternate a b c a b c ... so that clock drift hits all alike.
For the per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python tools/ledger_time.py --only b` (a run of its own).
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

    def league(**kw):
        env = crl.make_envs("cPongDouble-v0", num_envs=n, log_dir=None, seed=1, resized_dim=42, frame_stack=None)
        w = LeagueEnvWrapper(env, n, NAMES, seed=3, resample_on_done=True, **kw)
        w.reset()
        w.reset_opponent()
        return w

    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.randint(0, 3, (args.steps, n), generator=g, device="cuda", dtype=torch.int32)
    runs = {}
    for key, kw, pfsp_every in (("a league, uniform redraws", {}, 0), ("b league + ledger, weighted redraws", dict(ledger=True), 0),
                                ("c b + pfsp_weights every 10 steps", dict(ledger=True), 10)):
        if not args.only or key[0] in args.only:
            runs[key] = (league(**kw), pfsp_every)

    def rep(w, pfsp_every):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for t in range(args.steps):
            w.step_device(acts[t])
            if pfsp_every and t % pfsp_every == 0:
                w.ledger.pfsp_weights("hard", 2, 1)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps, (time.perf_counter() - t0) * 1e3 / args.steps

    for w, p in runs.values():  # warm-up
        rep(w, p)
    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, (w, p) in runs.items():
            ms[k].append(rep(w, p))
    res = {"envs": n, "steps_per_rep": args.steps, "reps": args.reps, "device": torch.cuda.get_device_name(0), "runs": {}}
    for k, v in ms.items():
        dev, wall = [x[0] for x in v], [x[1] for x in v]
        res["runs"][k] = {"device_ms_per_step_median": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
                          "wall_ms_per_step_median": statistics.median(wall), "all_device_ms": dev}
        print(f"{k:40s} {statistics.median(dev) * 1e3:9.1f} us/step device (min {min(dev) * 1e3:.1f}, max {max(dev) * 1e3:.1f}), "
              f"{statistics.median(wall) * 1e3:9.1f} us/step wall, {n / statistics.median(wall) / 1e3:.2f} M env-steps/s")
    for k, (w, _) in runs.items():
        res["runs"][k]["counts"] = dict(zip(NAMES, w.counts().tolist()))
        if w.ledger is not None:
            c = w.ledger.counters()
            res["runs"][k]["episodes"] = dict(zip(NAMES, c["episodes"].tolist()))
            res["runs"][k]["weights"] = w.ledger.weights().tolist()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for w, _ in runs.values():
        w.close()


if __name__ == "__main__":
    main()

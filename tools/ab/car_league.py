"""What CarLeague.step adds to the CarRacing loop step (include/crl.h "car league"): ONE process, three variants of the step alternating
inside every repeat, device events around spans of --span steps, medians and spreads.

    python tools/ab/car_league.py [--envs 16384] [--span 50] [--repeats 9] [--warmup 2] [--out FILE.json]

  parent   drivers.act + policy.act_rollout + step_device(render=False): the loop step without a league
  league   the same + league.step(rewards, done): books and redraws in one launch, nothing waits for the host
  torch    the same + what a trainer does without the league: accumulate both returns, read which envs are done (a host wait), book them
           with index_add_, draw their next opponents with torch.multinomial and push both assignments with assign(1, ...)
All three step the same env, whose ``elapsed`` counters are staggered over [0, 1000) so that about envs / 1000 episodes end in every step,
as in a long run.  Also timed alone: --span back-to-back league.step calls (the kernel and its launch).  Needs a GPU; there is no
fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import competitive_rl_amd as crl  # noqa: E402
from competitive_rl_amd.rules import car_league_columns  # noqa: E402


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def weights(seed):
    rs = np.random.RandomState(seed)
    u = lambda shape, fan: (rs.uniform(-1, 1, shape) / np.sqrt(fan)).astype(np.float32)  # noqa: E731
    return dict(fc1_w=u((100, 21), 21), fc1_b=u((100,), 21), policy_w=u((2, 100), 100), policy_b=u((2,), 100), value_w=u((1, 100), 100),
                value_b=u((1,), 100), log_std=np.array([-0.5, -0.5], np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--span", type=int, default=50, help="steps per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("car_league.py measures on the GPU; none is visible")
    n, k = args.envs, args.span
    env = crl.HipCarVecEnv(n, seed=0, done_policy="car0")
    policy, drivers = crl.CarPolicy(env, seed=0), crl.CarDrivers(env, seed=0)
    policy.add_network("learner", weights(0))
    policy.add_network("snapshot", weights(1))
    policy.assign(0, "learner")
    league = crl.CarLeague(env, policy, drivers, seed=0)
    league.add_style("RANDOM"), league.add_style("RULE_BASED"), league.add_network("snapshot")
    table = np.array([1, 3, 2], np.uint32)
    league.set_weights(table)
    acts, obs = torch.zeros((n, 2, 2), device="cuda"), torch.empty((n, 2, 21), device="cuda")
    env.reset()
    st = env.get_state()
    st["elapsed"][:] = (np.arange(n) * 1000) // n  # about n / 1000 episodes end in every step
    env.set_state(st)
    league.reset_assignment()

    # the torch leg's own books
    net_of, style_of = (torch.from_numpy(x).cuda() for x in car_league_columns(league.pool(), np.arange(3)))
    t_agent = league.assignment().to(torch.int64)
    t_ret, t_len = torch.zeros((n, 2), device="cuda"), torch.zeros((n,), dtype=torch.int64, device="cuda")
    t_counters = torch.zeros((7, 16), dtype=torch.int64, device="cuda")
    t_w = torch.from_numpy(table.astype(np.float32)).cuda()

    def base_step():
        drivers.act(acts)
        policy.act_rollout(acts, obs_out=obs)
        return env.step_device(acts, render=False)

    def parent_leg():
        for _ in range(k):
            base_step()

    def league_leg():
        for _ in range(k):
            _, rew, done = base_step()
            league.step(rew, done)

    def torch_leg():
        nonlocal t_ret, t_len
        for _ in range(k):
            _, rew, done = base_step()
            t_ret += rew
            t_len += 1
            idx = torch.nonzero(done).reshape(-1)  # (the host waits here: the count decides what is launched next)
            if idx.numel():
                a, r = t_agent[idx], t_ret[idx]
                won, lost = r[:, 0] > r[:, 1], r[:, 0] < r[:, 1]
                q = torch.round(r.double() * 256.0).to(torch.int64)
                rows = (torch.ones_like(a), won.long(), lost.long(), (~won & ~lost).long(), q[:, 0], q[:, 1], t_len[idx])
                for plane, v in enumerate(rows):
                    t_counters[plane].index_add_(0, a, v)
                t_agent[idx] = torch.multinomial(t_w, idx.numel(), replacement=True)
                t_ret[idx], t_len[idx] = 0.0, 0
                policy.assign(1, net_of[t_agent]), drivers.assign(1, style_of[t_agent])

    rew0, done0 = env._rew.clone(), env._done.clone()

    def kernel_leg():
        for _ in range(k):
            league.step(rew0, done0, redraw=True)

    legs = {"parent": parent_leg, "league": league_leg, "torch": torch_leg}
    order = list(legs)
    for name in order:
        for _ in range(args.warmup):
            legs[name]()
            torch.cuda.synchronize()
    ms = {name: [] for name in order}
    for r in range(args.repeats):
        shift = r % len(order)
        for name in order[shift:] + order[:shift]:
            ms[name].append(span(legs[name]) / k)
    booked = int(league.counters()["episodes"].sum())  # (what the three legs' steps ended; the span below books the last flags again)
    for _ in range(args.warmup):
        kernel_leg()
    torch.cuda.synchronize()
    ms["league.step alone"] = [span(kernel_leg) / k for _ in range(args.repeats)]
    med = {name: float(np.median(v)) for name, v in ms.items()}
    spread = {name: float((max(v) - min(v)) / np.median(v)) for name, v in ms.items()}
    for name in ms:
        print("%-18s median %.4f ms / step  spread %.2f %%  repeats %s" % (name, med[name], 100 * spread[name], " ".join("%.4f" % x for x in ms[name])),
              flush=True)
    # the added time: paired differences inside each repeat (the three legs of a repeat ran back to back)
    add_league = [1e3 * (a - b) for a, b in zip(ms["league"], ms["parent"])]
    add_torch = [1e3 * (a - b) for a, b in zip(ms["torch"], ms["parent"])]
    out = {"envs": n, "span": k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "ms_per_step": ms, "median_ms": med, "spread": spread,
           "added_us_league": {"median": float(np.median(add_league)), "min": float(min(add_league)), "max": float(max(add_league))},
           "added_us_torch": {"median": float(np.median(add_torch)), "min": float(min(add_torch)), "max": float(max(add_torch))},
           "league_step_alone_us": 1e3 * med["league.step alone"],
           "share_of_parent_step": float(np.median(add_league)) / (1e3 * med["parent"]),
           "torch_step_over_league_step": med["torch"] / med["league"],
           "episodes_booked": booked, "episodes_booked_torch": int(t_counters[0].sum())}
    print("league.step adds %.1f us (paired, min %.1f max %.1f) = %.2f %% of the parent's %.1f us step; alone %.1f us per call" % (
        out["added_us_league"]["median"], out["added_us_league"]["min"], out["added_us_league"]["max"], 100 * out["share_of_parent_step"],
        1e3 * med["parent"], out["league_step_alone_us"]))
    print("the torch equivalent adds %.1f us (min %.1f max %.1f); torch step / league step = %.2f (spreads %.2f %% + %.2f %%)" % (
        out["added_us_torch"]["median"], out["added_us_torch"]["min"], out["added_us_torch"]["max"], out["torch_step_over_league_step"],
        100 * spread["torch"], 100 * spread["league"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    league.close(), drivers.close(), policy.close(), env.close()


if __name__ == "__main__":
    main()

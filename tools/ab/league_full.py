"""What serving the full-size ActorCritic per env costs: the list launches of csrc/pong_policy_full.hip (crl_league_act with a
CRL_POOL_KIND_FULL agent) beside the dense launch of crl_policy_act, in ONE process, legs alternating inside every repeat.

    python tools/ab/league_full.py [--envs 65536] [--steps 50] [--repeats 5] [--warmup 10] [--out FILE.json]

Legs (device time per call between two events on the stream, the mean over `steps` calls; one figure per repeat):
  a        crl_policy_act of a dense full-size Policy (the existing path)
  a4       the same for a dense Policy of envs / 4 envs: what a quarter of the batch costs on the dense path (conv3 then runs one
           workgroup per CU instead of four, so it is more than a / 4)
  b        crl_league_act, pool [RULE_BASED, BIG], every env on BIG
  c        crl_league_act, pool [RULE_BASED, WEAK, MEDIUM, BIG], a quarter of the envs each (env i on agent i mod 4)
  d        crl_league_act, pool [RULE_BASED, WEAK, MEDIUM], a third each (env i on agent i mod 3)
  d_idle   the same pool and assignment with an unassigned BIG beside it
  c_light  pool [RULE_BASED, WEAK, MEDIUM] with c's assignment of those three (BIG's quarter on RULE_BASED): what c costs without BIG
Printed: each leg's repeats, median and spread (max - min) / median, and the ratios b / a, c against a / 4 + c_light and a4 + c_light, d_idle - d.
Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from competitive_rl_amd import _native as N  # noqa: E402
from competitive_rl_amd import spaces  # noqa: E402
from competitive_rl_amd.league import LeagueEnvWrapper  # noqa: E402
from competitive_rl_amd.policy_serving import Policy, _random_full_weights  # noqa: E402


class Host:
    """What LeagueEnvWrapper reads of the env it wraps; the legs call crl_league_act on made-up frames and never step an env."""
    R, env_id_base, observation_space, action_space = 42, 0, [None], [None]

    def __init__(self):
        self.device = torch.device("cuda", torch.cuda.current_device())

    def close(self):
        pass


def league(n, names, big, assign):
    lg = LeagueEnvWrapper(Host(), n, names, seed=5)
    if big is not None:
        lg.add_full_agent("BIG", big)
    lg.set_opponents(assign)
    return lg


def league_call(lg, frame):
    """crl_league_act alone (LeagueEnvWrapper._fill_actions without the copy of the caller's own actions)"""
    N.check(lg._L.crl_league_act(lg._h, C.c_void_p(frame.data_ptr()), frame.stride(0), C.c_void_p(lg._act.data_ptr() + 4), 2, None, lg._stream()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("league_full.py measures on the GPU; none is visible")
    n = args.envs
    torch.manual_seed(0)
    w = _random_full_weights()
    frames = [(torch.randint(0, 256, (n, 1, 42, 42), device="cuda", dtype=torch.uint8) * (torch.rand((n, 1, 42, 42), device="cuda") > 0.7)).contiguous()
              for _ in range(4)]
    i = np.arange(n)
    pol = Policy(spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3), n, use_light_model=False, weights=w)
    light = ["RULE_BASED", "WEAK", "MEDIUM"]
    lgs = {"b": league(n, ["RULE_BASED"], w, np.ones(n, np.int64)),
           "c": league(n, light, w, i % 4),
           "d": league(n, light, None, i % 3),
           "d_idle": league(n, light, w, i % 3),
           "c_light": league(n, light, None, np.where(i % 4 == 3, 0, i % 4))}
    assert lgs["b"].counts().tolist() == [0, n] and lgs["d_idle"].counts()[3] == 0 and lgs["c"].counts()[3] == n // 4
    pol4 = Policy(spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3), n // 4, use_light_model=False, weights=w)
    legs = {"a": lambda f: pol.act_device(f), "a4": lambda f: pol4.act_device(f[:n // 4])}
    for k, lg in lgs.items():
        legs[k] = (lambda f, lg=lg: league_call(lg, f.reshape(n, 42, 42)))
    order = list(legs)
    for k in order:
        for t in range(args.warmup):
            legs[k](frames[t % 4])
    torch.cuda.synchronize()
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:  # (another leg goes first in every repeat)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(args.steps):
                legs[k](frames[t % 4])
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in order:
        print("%-8s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])))
    out = {"envs": n, "steps": args.steps, "repeats": args.repeats, "ms": ms, "median_ms": med, "spread": spread,
           "b_over_a": med["b"] / med["a"], "c_ms": med["c"], "quarter_a_plus_c_light_ms": med["a"] / 4 + med["c_light"],
           "a4_plus_c_light_ms": med["a4"] + med["c_light"],
           "idle_cost_ms": med["d_idle"] - med["d"], "device": torch.cuda.get_device_name(0)}
    print("b / a = %.4f   c = %.4f ms against a / 4 + c_light = %.4f ms and a4 + c_light = %.4f ms   d_idle - d = %+.4f ms" % (
        out["b_over_a"], out["c_ms"], out["quarter_a_plus_c_light_ms"], out["a4_plus_c_light_ms"], out["idle_cost_ms"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    pol.close(), pol4.close()
    for lg in lgs.values():
        lg.close()


if __name__ == "__main__":
    main()

"""What serving a learner costs (include/crl.h "rollout heads"): crl_policy_act_rollout with values and log-probs beside crl_policy_act
(the unchanged kernels), the reset-mask launch, a weight reload between two act calls, and -- for scale -- a torch forward pass of the
same two networks on a float32 stack, which is what a trainer pays without these kernels.  ONE process, legs alternating inside every
repeat.

    python tools/ab/rollout_heads.py [--envs 65536] [--steps 50] [--repeats 5] [--warmup 10] [--torch] [--out FILE.json]

Legs (device time per call between two events on the stream, the mean over `steps` calls; one figure per repeat), each for the
LightActorCritic (`light_`) and the full-size ActorCritic (`full_`), greedy and at temperature 1 (`_T1`):
  *_act            crl_policy_act
  *_rollout        crl_policy_act_rollout with values and log-probs, no reset flags
  light_mask0      light_rollout with a reset tensor that has no flag set (the mask launch: every wavefront leaves after its ballot)
  light_mask64     ... with one env in 64 flagged (1 024 rings zeroed per call)
  *_reload         load_weights followed by crl_policy_act: what a reload between two act calls adds is this minus *_act
--torch runs ONLY the torch legs (a separate invocation: torch's convolutions bring their own library start-up):
  torch_light / torch_full   torch.no_grad() forward (logits and value) of the same networks on a float32 (envs, 4, 42, 42) stack
Printed: each leg's repeats, median and spread (max - min) / median, and the differences named above.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from competitive_rl_amd import spaces  # noqa: E402
from competitive_rl_amd.policy_serving import Policy, _random_full_weights, _random_light_weights  # noqa: E402


def with_critic(w, features, seed):
    rs = np.random.RandomState(seed)
    return {**w, "critic_w": (rs.standard_normal((1, features)) * 0.05).astype(np.float32), "critic_b": np.array([0.1], np.float32)}


def torch_nets():
    import torch.nn as nn

    class Light(nn.Module):  # utils/network.py:73-93
        def __init__(self):
            super().__init__()
            self.conv1, self.conv2 = nn.Conv2d(4, 16, 4, 2), nn.Conv2d(16, 16, 2, 2)
            self.actor_linear, self.critic_linear = nn.Linear(1600, 3), nn.Linear(1600, 1)

        def forward(self, x):
            x = torch.relu(self.conv1(x / 255.0))
            x = torch.relu(self.conv2(x)).flatten(1)
            return self.actor_linear(x), self.critic_linear(x)

    class Full(nn.Module):  # utils/network.py:14-50
        def __init__(self):
            super().__init__()
            self.conv1, self.conv2, self.conv3 = nn.Conv2d(4, 16, 4, 2), nn.Conv2d(16, 32, 4, 2, 2), nn.Conv2d(32, 256, 11)
            self.actor_linear, self.critic_linear = nn.Linear(256, 3), nn.Linear(256, 1)

        def forward(self, x):
            x = torch.relu(self.conv1(x / 255.0))
            x = torch.relu(self.conv3(torch.relu(self.conv2(x)))).flatten(1)
            return self.actor_linear(x), self.critic_linear(x)

    return {"torch_light": Light().cuda().eval(), "torch_full": Full().cuda().eval()}


def measure(legs, frames, args):
    order = list(legs)
    for k in order:
        for t in range(args.warmup):
            legs[k](frames[t % len(frames)])
        torch.cuda.synchronize()
        print("warmed up", k, flush=True)
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:  # (another leg goes first in every repeat)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(args.steps):
                legs[k](frames[t % len(frames)])
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in order:
        print("%-18s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])), flush=True)
    return ms, med, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_heads.py measures on the GPU; none is visible")
    n = args.envs
    torch.manual_seed(0)
    out = {"envs": n, "steps": args.steps, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    if args.torch:
        nets = torch_nets()
        stacks = [torch.randint(0, 256, (n, 4, 42, 42), device="cuda", dtype=torch.uint8).float() for _ in range(2)]

        def leg(net):
            def run(x):
                with torch.no_grad():
                    net(x)
            return run

        ms, med, spread = measure({k: leg(v) for k, v in nets.items()}, stacks, args)
    else:
        frames = [(torch.randint(0, 256, (n, 1, 42, 42), device="cuda", dtype=torch.uint8) * (torch.rand((n, 1, 42, 42), device="cuda") > 0.7)).contiguous()
                  for _ in range(4)]
        box, disc = spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3)
        wl = [with_critic(_random_light_weights(), 1600, s) for s in (1, 2)]
        wf = [with_critic(_random_full_weights(), 256, s) for s in (3, 4)]
        pols, legs = [], {}
        none = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        some = (torch.arange(n, device="cuda") % 64 == 17).to(torch.uint8)
        for tag, light, w in (("light", True, wl), ("full", False, wf)):
            for style in ("", "_T1"):
                p = Policy(box, disc, n, use_light_model=light, weights=w[0])
                if style:
                    p.set_sampling(1.0, 0.0, seed=9)
                pols.append(p)
                legs[tag + "_act" + style] = (lambda f, p=p: p.act_device(f))
                legs[tag + "_rollout" + style] = (lambda f, p=p: p.act_rollout(f))
                if not style:
                    state = {"i": 0}

                    def reload(f, p=p, w=w, state=state):
                        state["i"] ^= 1
                        p.load_weights(w[state["i"]])
                        p.act_device(f)

                    legs[tag + "_reload"] = reload
                    if light:
                        legs["light_mask0"] = (lambda f, p=p: p.act_rollout(f, reset=none))
                        legs["light_mask64"] = (lambda f, p=p: p.act_rollout(f, reset=some))
        ms, med, spread = measure(legs, frames, args)
        for tag in ("light", "full"):
            for style in ("", "_T1"):
                a, r = med[tag + "_act" + style], med[tag + "_rollout" + style]
                out[tag + style + "_rollout_over_act"] = r / a
                print("%s%s: rollout / act = %.4f (%+.4f ms)" % (tag, style, r / a, r - a))
            out[tag + "_reload_cost_ms"] = med[tag + "_reload"] - med[tag + "_act"]
            print("%s: a reload between two act calls adds %+.4f ms" % (tag, out[tag + "_reload_cost_ms"]))
        out["mask0_cost_ms"], out["mask64_cost_ms"] = med["light_mask0"] - med["light_rollout"], med["light_mask64"] - med["light_rollout"]
        print("reset mask: no flag %+.4f ms, one env in 64 %+.4f ms" % (out["mask0_cost_ms"], out["mask64_cost_ms"]))
        for p in pols:
            p.close()
    out.update({"ms": ms, "median_ms": med, "spread": spread})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

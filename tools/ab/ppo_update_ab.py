"""What one PPO minibatch update costs (include/crl.h "ppo update"): ONE process, the two legs alternating inside every repeat, device
events around each leg, medians and spreads.

    python tools/ab/ppo_update_ab.py [--envs 65536] [--steps 32] [--batch 262144] [--repeats 7] [--warmup 2] [--torch-chunk 32768] [--legs device,torch]
                                     [--out FILE.json]

  device   learner.grad(storage, idx) + learner.step(): the gradient straight from the stored uint8 planes, reduce, clip + Adam
  torch    the restatement a trainer around the library runs today: storage.gather(idx) as float32, a torch LightActorCritic (restated
           below from utils/network.py:73-93) forward, the same loss, backward(), clip_grad_norm_ and Adam.step().  In chunks of
           --torch-chunk samples whose gradients accumulate: one forward over 131 072 or more stacks did not finish its first
           call within five minutes on the MI355X (docs/LAB_NOTES_ppo_update.md)
Both legs see the same storage, the same idx and the same starting weights.  The device leg's share of the fp32 matrix peak counts the
matrix instructions the gradient kernel issues (1 500 v_mfma_f32_16x16x4_f32 per sample: 500 forward, 400 conv1 again, 600 backward) at
2 048 FLOP each (16 x 16 x 4 multiply-adds) against 256 CUs x 4 SIMDs x 64 FLOP / clk (MI355X_MICROARCH) at the clock given by --ghz.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from competitive_rl_amd.policy_serving import _random_light_weights  # noqa: E402
from competitive_rl_amd.ppo import LightPPO  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import PPO_DEFAULTS  # noqa: E402


class LightActorCritic(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(4, 16, 4, stride=2), nn.Conv2d(16, 16, 2, stride=2)
        self.actor_linear, self.critic_linear = nn.Linear(1600, 3), nn.Linear(1600, 1)
        with torch.no_grad():
            for mod, k in ((self.conv1, "conv1"), (self.conv2, "conv2"), (self.actor_linear, "actor"), (self.critic_linear, "critic")):
                mod.weight.copy_(torch.from_numpy(w[k + "_w"])), mod.bias.copy_(torch.from_numpy(w[k + "_b"]))

    def forward(self, x):
        x = F.relu(self.conv1(x / 255.0))
        x = F.relu(self.conv2(x)).reshape(x.shape[0], -1)
        return self.actor_linear(x), self.critic_linear(x).reshape(-1)


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--torch-chunk", type=int, default=32768, help="samples per forward / backward of the torch leg (gradients accumulate)")
    ap.add_argument("--legs", default="device,torch", help="the legs to run, e.g. `device` alone where the torch leg does not fit")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_update_ab.py measures on the GPU; none is visible")
    n, steps, b = args.envs, args.steps, args.batch
    h = PPO_DEFAULTS
    w = {**_random_light_weights(), "critic_w": (np.random.RandomState(1).standard_normal((1, 1600)) * 0.05).astype(np.float32),
         "critic_b": np.array([0.1], np.float32)}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    st = RolloutStorage(steps, n)
    none = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for t in range(steps):
        obs = torch.randint(0, 256, (n, 1, 42, 42), device="cuda", dtype=torch.uint8, generator=g)
        st.record(obs, torch.rand(n, device="cuda", generator=g) < 0.01, torch.randn(n, device="cuda", generator=g),
                  torch.randint(0, 3, (n,), device="cuda", dtype=torch.int32, generator=g), -1.1 + 0.1 * torch.randn(n, device="cuda", generator=g))
        st.outcome(torch.randn(n, device="cuda", generator=g), none)
    st.finish()
    idx = [torch.randint(0, steps * n, (b,), device="cuda", generator=g) for _ in range(2)]
    learner = LightPPO(w)
    net = LightActorCritic(w).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=h["lr"], betas=h["betas"], eps=h["eps"])
    chunk = min(b, args.torch_chunk)
    batch = st.empty_batch(chunk)

    def device_leg(c):
        learner.grad(st, idx[c])
        learner.step()

    def torch_leg(c):
        opt.zero_grad(set_to_none=True)
        for lo in range(0, b, chunk):  # gradients add up over the chunks: the same mean over B, one optimiser step
            i = idx[c][lo:lo + chunk]
            bt = st.gather(i, out=batch) if i.numel() == chunk else st.gather(i)
            logits, v = net(bt.obs)
            lp_all = torch.log_softmax(logits, dim=1)
            logp = lp_all.gather(1, bt.actions.long()[:, None]).reshape(-1)
            ratio = torch.exp(logp - bt.old_log_probs)
            policy = -torch.minimum(ratio * bt.advantages, torch.clamp(ratio, 1 - h["clip"], 1 + h["clip"]) * bt.advantages)
            loss = (policy + h["vf_coef"] * 0.5 * (bt.returns - v) ** 2 + h["ent_coef"] * (lp_all.exp() * lp_all).sum(1)).sum() / b
            loss.backward()
        nn.utils.clip_grad_norm_(net.parameters(), h["max_grad_norm"])
        opt.step()

    legs = {k: fn for k, fn in (("device", device_leg), ("torch", torch_leg)) if k in args.legs.split(",")}
    order = list(legs)
    for k in order:
        for c in range(args.warmup):
            legs[k](c % 2)
            torch.cuda.synchronize()
            print("warm-up round", c, "of", k, flush=True)
        print("warmed up", k, flush=True)
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:
            ms[k].append(span(lambda: legs[k](r % 2)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in order:
        print("%-8s median %.3f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.3f" % x for x in ms[k])), flush=True)
    peak = 256 * 4 * 64 * args.ghz * 1e9
    out = {"envs": n, "steps": steps, "batch": b, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "ms": ms, "median_ms": med,
           "spread": spread}
    if "device" in med:
        out["matrix_peak_share"] = b * 1500 * 2048 / (med["device"] * 1e-3) / peak
        out["stats"] = list(learner.stats())
        print("the device leg issues %.1f %% of the fp32 matrix peak at %.1f GHz" % (100 * out["matrix_peak_share"], args.ghz))
    if len(med) == 2:
        out["torch_over_device"], out["combined_spread"] = med["torch"] / med["device"], spread["device"] + spread["torch"]
        print("torch / device = %.2f (the two legs' combined spread %.2f %%)" % (out["torch_over_device"], 100 * out["combined_spread"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

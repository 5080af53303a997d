"""What one PPO minibatch update of the full-size ActorCritic costs (include/crl.h "ppo update, full size"): ONE process, the legs alternating
inside every repeat, device events around each leg, medians and spreads.

    python tools/ab/ppo_full_update_ab.py [--envs 16384] [--steps 16] [--batch 65536] [--repeats 7] [--warmup 2] [--torch-chunks 2048,4096,8192]
                                          [--scratch-rows 0] [--legs device,torch] [--out FILE.json]

  device   learner.grad(storage, idx) + learner.step(): the gradient straight from the stored uint8 planes, clip + Adam
  torch    what a trainer around the library runs today: storage.gather(idx) as float32, the reference's ActorCritic (restated below from
           utils/network.py:14-50) forward, the same loss, backward(), clip_grad_norm_ and Adam.step(), in chunks whose gradients
           accumulate.  One leg per entry of --torch-chunks; the fastest median is the baseline.
All legs see the same storage, the same idx and the same starting weights.  The device leg's share of the fp32 matrix peak counts the
v_mfma_f32_16x16x4_f32 it issues per sample (conv2 1 024, conv3 968, gW3 968, dz2 968, gW2 992, da1 896, gW1 400 = 6 216; conv1's bf16
instructions, twice 150, are left out) at 2 048 FLOP each against 256 CUs x 4 SIMDs x 64 FLOP / clk at the clock given by --ghz.
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

from competitive_rl_amd.policy_serving import _random_full_weights  # noqa: E402
from competitive_rl_amd.ppo import FullPPO  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import PPO_DEFAULTS  # noqa: E402

MFMA_PER_SAMPLE = 1024 + 968 + 968 + 968 + 992 + 896 + 400


class ActorCritic(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.conv1, self.conv2, self.conv3 = nn.Conv2d(4, 16, 4, stride=2), nn.Conv2d(16, 32, 4, stride=2, padding=2), nn.Conv2d(32, 256, 11)
        self.actor_linear, self.critic_linear = nn.Linear(256, 3), nn.Linear(256, 1)
        with torch.no_grad():
            for mod, k in ((self.conv1, "conv1"), (self.conv2, "conv2"), (self.conv3, "conv3"), (self.actor_linear, "actor"), (self.critic_linear, "critic")):
                mod.weight.copy_(torch.from_numpy(w[k + "_w"])), mod.bias.copy_(torch.from_numpy(w[k + "_b"]))

    def forward(self, x):
        x = F.relu(self.conv1(x / 255.0))
        x = F.relu(self.conv2(x))
        x = F.relu(self.conv3(x)).reshape(x.shape[0], -1)
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
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--torch-chunks", default="2048,4096,8192", help="samples per forward / backward of the torch legs (gradients accumulate)")
    ap.add_argument("--scratch-rows", type=int, default=0, help="the learner's scratch_rows (0: its default)")
    ap.add_argument("--legs", default="device,torch")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_full_update_ab.py measures on the GPU; none is visible")
    n, steps, b = args.envs, args.steps, args.batch
    h = PPO_DEFAULTS
    torch.manual_seed(0)
    w = {**_random_full_weights(), "critic_w": (np.random.RandomState(1).standard_normal((1, 256)) * 0.05).astype(np.float32),
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
    want = args.legs.split(",")
    legs = {}
    if "device" in want:
        learner = FullPPO(w, scratch_rows=args.scratch_rows or None)

        def device_leg(c):
            learner.grad(st, idx[c])
            learner.step()

        legs["device"] = device_leg

    def torch_leg_of(chunk):
        net = ActorCritic(w).cuda()
        opt = torch.optim.Adam(net.parameters(), lr=h["lr"], betas=h["betas"], eps=h["eps"])
        batch = st.empty_batch(chunk)

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

        return torch_leg

    if "torch" in want:
        for c in args.torch_chunks.split(","):
            legs["torch%d" % int(c)] = torch_leg_of(min(b, int(c)))
    order = list(legs)
    for k in order:
        for c in range(args.warmup):
            legs[k](c % 2)
            torch.cuda.synchronize()
            print("warm-up round", c, "of", k, flush=True)
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:
            ms[k].append(span(lambda: legs[k](r % 2)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in order:
        print("%-10s median %.3f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.3f" % x for x in ms[k])), flush=True)
    peak = 256 * 4 * 64 * args.ghz * 1e9
    out = {"envs": n, "steps": steps, "batch": b, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "ms": ms, "median_ms": med,
           "spread": spread}
    if "device" in med:
        out["matrix_peak_share"] = b * MFMA_PER_SAMPLE * 2048 / (med["device"] * 1e-3) / peak
        out["stats"] = list(learner.stats())
        print("the device leg issues %.1f %% of the fp32 matrix peak at %.1f GHz" % (100 * out["matrix_peak_share"], args.ghz))
    torch_legs = [k for k in med if k.startswith("torch")]
    if "device" in med and torch_legs:
        best = min(torch_legs, key=lambda k: med[k])
        out["baseline"], out["torch_over_device"], out["combined_spread"] = best, med[best] / med["device"], spread["device"] + spread[best]
        out["requirement_met"] = med["device"] <= med[best] * (1 + out["combined_spread"])
        print("baseline %s: torch / device = %.2f (the two legs' combined spread %.2f %%); device not slower: %s" %
              (best, out["torch_over_device"], 100 * out["combined_spread"], out["requirement_met"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

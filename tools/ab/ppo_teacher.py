"""What a teacher costs on a PPO minibatch update (include/crl.h "ppo update, teacher targets"): ONE process, the legs alternating inside
every repeat, device events around each leg, medians and spreads.

    python tools/ab/ppo_teacher.py [--full] [--envs N] [--steps T] [--batch B] [--repeats 7] [--warmup 2] [--legs plain,logits,labels] [--out FILE.json]

  plain    learner.grad(storage, idx) + learner.step(): the launches of before.  Run with --legs plain at the parent commit and at
           the branch, this leg is the parent-against-branch comparison (the plain kernels are the parent's instruction for instruction)
  logits   the same with Teacher(logits=(T, N, 3), temperature=2, coef=1, policy_term=False)
  labels   the same with Teacher(labels=(T, N) of which a fifth are -1, value_targets=(T, N), policy_term=False)
and, where the library has it, `rule_labels` at --label-envs envs: the launch alone, 200 calls between two events.
Defaults are the README's shapes: 262 144 samples of a 65 536 x 32 storage (light), 65 536 of 16 384 x 16 with --full.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from competitive_rl_amd import ppo as PPO  # noqa: E402
from competitive_rl_amd.policy_serving import _random_light_weights  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def full_weights(seed=2024):
    rs = np.random.RandomState(seed)
    shapes = dict(conv1_w=(16, 4, 4, 4), conv1_b=(16,), conv2_w=(32, 16, 4, 4), conv2_b=(32,), conv3_w=(256, 32, 11, 11), conv3_b=(256,),
                  actor_w=(3, 256), actor_b=(3,), critic_w=(1, 256), critic_b=(1,))
    return {k: (rs.standard_normal(s) / np.sqrt(max(1, int(np.prod(s[1:]))))).astype(np.float32) for k, s in shapes.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--envs", type=int, default=0)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="plain,logits,labels")
    ap.add_argument("--label-envs", type=int, default=65536)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_teacher.py measures on the GPU; none is visible")
    n = args.envs or (16384 if args.full else 65536)
    steps = args.steps or (16 if args.full else 32)
    b = args.batch or (65536 if args.full else 262144)
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
    if args.full:
        learner = PPO.FullPPO(full_weights())
    else:
        learner = PPO.LightPPO({**_random_light_weights(), "critic_w": (np.random.RandomState(1).standard_normal((1, 1600)) * 0.05).astype(np.float32),
                                "critic_b": np.array([0.1], np.float32)})
    teachers = {}
    if hasattr(PPO, "Teacher"):
        labels = torch.randint(0, 3, (steps, n), device="cuda", dtype=torch.int32, generator=g)
        labels.reshape(-1)[::5] = -1
        teachers["logits"] = PPO.Teacher(logits=torch.randn((steps, n, 3), device="cuda", generator=g), temperature=2.0, coef=1.0, policy_term=False)
        teachers["labels"] = PPO.Teacher(labels=labels, value_targets=torch.randn((steps, n), device="cuda", generator=g), policy_term=False)

    def leg(name):
        def run(c):
            if name == "plain":
                learner.grad(st, idx[c])
            else:
                learner.grad(st, idx[c], teacher=teachers[name])
            learner.step()
        return run

    order = [k for k in args.legs.split(",") if k == "plain" or k in teachers]
    legs = {k: leg(k) for k in order}
    for k in order:
        for c in range(args.warmup):
            legs[k](c % 2)
            torch.cuda.synchronize()
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:
            ms[k].append(span(lambda: legs[k](r % 2)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in order:
        print("%-8s median %.3f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.3f" % x for x in ms[k])), flush=True)
    out = {"full": args.full, "envs": n, "steps": steps, "batch": b, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "ms": ms,
           "median_ms": med, "spread": spread}
    for k in order:
        if k != "plain" and "plain" in med:
            out[k + "_over_plain"] = med[k] / med["plain"]
            print("%s / plain = %.4f (the two legs' combined spread %.2f %%)" % (k, out[k + "_over_plain"], 100 * (spread[k] + spread["plain"])))
    from competitive_rl_amd.vec_env import HipPongVecEnv
    if hasattr(HipPongVecEnv, "rule_labels") and args.label_envs > 0:
        env = HipPongVecEnv(args.label_envs, seed=0, mode="wrapped", resized_dim=42, output="torch")
        env.reset()
        buf = torch.empty((args.label_envs,), dtype=torch.int32, device="cuda")
        us = []
        for r in range(args.repeats + 1):
            def calls():
                for _ in range(200):
                    env.rule_labels(seat=0, out=buf)
            t = span(calls) * 1000.0 / 200
            if r:
                us.append(t)
        out["rule_labels_us"], out["rule_labels_envs"] = us, args.label_envs
        print("rule_labels at %d envs: median %.2f us per call (spread %.2f %%)" % (args.label_envs, float(np.median(us)), 100 * (max(us) - min(us)) / np.median(us)))
        env.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

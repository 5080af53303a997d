"""What the teacher term costs the CarRacing learner's update (include/crl.h "car ppo update, teacher targets"): ONE process, the legs
alternating inside every repeat, device events around each leg, medians and spreads.

    python tools/ab/car_ppo_teacher.py [--envs 16384] [--steps 32] [--batch 262144] [--repeats 9] [--warmup 3] [--out FILE.json]

  plain      learner.grad(storage, idx) + learner.step(): the plain instantiation, the leg ``device`` of tools/ab/car_ppo.py
  mse        ... with teacher=CarTeacher(target, loss="mse", policy_term=False): the cloning loss of examples/clone_car_driver.py
  ce-values  ... with teacher=CarTeacher(target, log_std=..., value_targets=...): the Gaussian cross-entropy, every load the teacher
             instantiation can make (8 + 4 bytes per sample beside the 128-byte line)
All legs see the same storage (the 16 384-env x 2-car x 32-step storage of tools/ab/car_ppo.py, filled by the real loop), the same idx
and a learner of their own at the same starting weights; the targets are what a RULE_BASED ``CarDrivers`` (epsilon 0) answered in the
visited states.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import competitive_rl_amd as crl  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("car_ppo_teacher.py measures on the GPU; none is visible")
    n, steps, b = args.envs, args.steps, args.batch
    rs = np.random.RandomState(0)
    u = lambda shape, fan: (rs.uniform(-1, 1, shape) / np.sqrt(fan)).astype(np.float32)  # noqa: E731
    w = dict(fc1_w=u((100, 21), 21), fc1_b=u((100,), 21), policy_w=u((2, 100), 100), policy_b=u((2,), 100), value_w=u((1, 100), 100),
             value_b=u((1,), 100), log_std=np.array([-0.5, -0.5], np.float32))
    env = crl.HipCarVecEnv(n, seed=0, done_policy="car0")
    policy = crl.CarPolicy(env, seed=0)
    policy.add_network("learner", w)
    policy.assign(0, "learner"), policy.assign(1, "learner")
    rule = crl.CarDrivers(env, seed=0)
    rule.assign(0, "RULE_BASED"), rule.assign(1, "RULE_BASED")
    st = crl.CarRolloutStorage(env, steps, cars=(0, 1))
    acts, obs = torch.zeros((n, 2, 2), device="cuda"), torch.empty((n, 2, 21), device="cuda")
    target = torch.zeros((steps, n, 2, 2), device="cuda")
    vtarget = torch.zeros((steps, n, 2), device="cuda")
    env.reset()
    st.begin()
    values, logp = policy.act_rollout(acts, obs_out=obs)
    for t in range(steps):
        rule.act(target[t])
        vtarget[t] = values
        st.record(t, policy, "learner", obs, acts, values, logp)
        _, rew, done = env.step_device(acts, render=False)
        st.outcome(t, rew, done)
        values, logp = policy.act_rollout(acts, obs_out=obs)
    st.finish(values)
    total = steps * n * 2
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    idx = [torch.randint(0, total, (b,), device="cuda", generator=g) for _ in range(2)]
    teachers = {"plain": None, "mse": crl.CarTeacher(target, loss="mse", policy_term=False),
                "ce-values": crl.CarTeacher(target, log_std=[-1.0, -1.0], value_targets=vtarget, coef=0.5)}
    learners = {k: crl.CarPPO(w) for k in teachers}

    def leg(k, c):
        learners[k].grad(st, idx[c], teacher=teachers[k])
        learners[k].step()

    order = list(teachers)
    for k in order:
        for c in range(args.warmup):
            leg(k, c % 2)
            torch.cuda.synchronize()
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        s = r % len(order)
        for k in order[s:] + order[:s]:
            ms[k].append(span(lambda: leg(k, r % 2)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in ms:
        print("%-10s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])), flush=True)
    out = {"envs": n, "steps": steps, "batch": b, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "ms": ms, "median_ms": med,
           "spread": spread, "teacher_stats": {k: list(learners[k].teacher_stats()) for k in order if teachers[k] is not None},
           "over_plain": {k: med[k] / med["plain"] for k in order if k != "plain"},
           "combined_spread": {k: spread[k] + spread["plain"] for k in order if k != "plain"}}
    for k in out["over_plain"]:
        print("%s / plain = %.3f (the two legs' combined spread %.2f %%)" % (k, out["over_plain"][k], 100 * out["combined_spread"][k]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

"""What the CarRacing learner's calls cost (include/crl.h "car rollout storage", "car ppo update"): ONE process, the two legs of the
update alternating inside every repeat, device events around each leg, medians and spreads.

    python tools/ab/car_ppo.py [--envs 16384] [--steps 32] [--batch 262144] [--repeats 9] [--warmup 3] [--out FILE.json]

  device   learner.grad(storage, idx) + learner.step(): the gradient straight from the sample lines, reduce, clip + Adam
  torch    what a trainer around CarPolicy runs without the learner: storage.gather(idx) feeding a torch MLP(21, 2) (restated below from
           utils/network.py:59-70, with a log_std parameter) with the same loss over the live samples, backward(), clip_grad_norm_ and
           Adam.step()
Both legs see the same storage, the same idx and the same starting weights.  Also timed, each as the median of --repeats spans of 20
calls: act_rollout (the yardstick of the serving call), record + outcome, and finish.  The storage is filled by the real loop: a
HipCarVecEnv stepped without frames.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import competitive_rl_amd as crl  # noqa: E402
from competitive_rl_amd.rules import CAR_PPO_DEFAULTS  # noqa: E402

LN_2PI = float(np.log(2 * np.pi))


class MLP(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.fc1, self.policy, self.value = nn.Linear(21, 100), nn.Linear(100, 2), nn.Linear(100, 1)
        self.log_std = nn.Parameter(torch.from_numpy(w["log_std"].copy()))
        with torch.no_grad():
            for mod, k in ((self.fc1, "fc1"), (self.policy, "policy"), (self.value, "value")):
                mod.weight.copy_(torch.from_numpy(w[k + "_w"])), mod.bias.copy_(torch.from_numpy(w[k + "_b"]))

    def forward(self, x):
        x = torch.relu(self.fc1(x))
        return self.policy(x), self.value(x).reshape(-1)


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
        raise SystemExit("car_ppo.py measures on the GPU; none is visible")
    n, steps, b, h = args.envs, args.steps, args.batch, CAR_PPO_DEFAULTS
    rs = np.random.RandomState(0)
    u = lambda shape, fan: (rs.uniform(-1, 1, shape) / np.sqrt(fan)).astype(np.float32)  # noqa: E731
    w = dict(fc1_w=u((100, 21), 21), fc1_b=u((100,), 21), policy_w=u((2, 100), 100), policy_b=u((2,), 100), value_w=u((1, 100), 100),
             value_b=u((1,), 100), log_std=np.array([-0.5, -0.5], np.float32))
    env = crl.HipCarVecEnv(n, seed=0, done_policy="car0")
    policy = crl.CarPolicy(env, seed=0)
    policy.add_network("learner", w)
    policy.assign(0, "learner"), policy.assign(1, "learner")
    st = crl.CarRolloutStorage(env, steps, cars=(0, 1))
    acts, obs = torch.zeros((n, 2, 2), device="cuda"), torch.empty((n, 2, 21), device="cuda")
    env.reset()
    st.begin()
    values, logp = policy.act_rollout(acts, obs_out=obs)
    for t in range(steps):
        st.record(t, policy, "learner", obs, acts, values, logp)
        _, rew, done = env.step_device(acts, render=False)
        st.outcome(t, rew, done)
        values, logp = policy.act_rollout(acts, obs_out=obs)
    st.finish(values)
    total = steps * n * 2
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    idx = [torch.randint(0, total, (b,), device="cuda", generator=g) for _ in range(2)]
    learner = crl.CarPPO(w)
    net = MLP(w).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=h["lr"], betas=h["betas"], eps=h["eps"])
    batch = st.empty_batch(b)

    def device_leg(c):
        learner.grad(st, idx[c])
        learner.step()

    def torch_leg(c):
        opt.zero_grad(set_to_none=True)
        bt = st.gather(idx[c], out=batch)
        mean, v = net(bt.obs)
        zz = (bt.actions - mean) / torch.exp(net.log_std)
        lp = (-0.5 * zz ** 2 - net.log_std).sum(1) - LN_2PI
        ratio = torch.exp(lp - bt.old_log_probs)
        pol = -torch.minimum(ratio * bt.advantages, torch.clamp(ratio, 1 - h["clip"], 1 + h["clip"]) * bt.advantages)
        ent = net.log_std.sum() + (1 + LN_2PI)
        live = bt.live.to(torch.float32)
        loss = ((pol + h["vf_coef"] * 0.5 * (bt.returns - v) ** 2 - h["ent_coef"] * ent) * live).sum() / live.sum().clamp(min=1)
        loss.backward()
        nn.utils.clip_grad_norm_(net.parameters(), h["max_grad_norm"])
        opt.step()

    legs = {"device": device_leg, "torch": torch_leg}
    order = list(legs)
    for k in order:
        for c in range(args.warmup):
            legs[k](c % 2)
            torch.cuda.synchronize()
    ms = {k: [] for k in order}
    for r in range(args.repeats):
        for k in order[r % 2:] + order[:r % 2]:
            ms[k].append(span(lambda: legs[k](r % 2)))
    # the per-step calls: 20 calls per span
    calls = 20

    def act_calls():
        for _ in range(calls):
            policy.act_rollout(acts, obs_out=obs)

    def record_outcome_calls():
        st.begin()
        for t in range(calls):
            st.record(t, policy, "learner", obs, acts, values, logp)
            st.outcome(t, rew, done)

    def finish_calls():
        for _ in range(calls):
            st.finish(values)

    small = {"act_rollout": act_calls, "record+outcome": record_outcome_calls, "finish": finish_calls}
    assert steps >= calls, "--steps must be at least 20: record + outcome is timed over 20 steps of one rollout"
    for k, fn in small.items():
        if k == "finish":  # (the record + outcome spans leave the rollout open: close it with its remaining steps)
            for t in range(calls, steps):
                st.record(t, policy, "learner", obs, acts, values, logp)
                st.outcome(t, rew, done)
            st.finish(values)
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms[k] = [span(fn) / calls for _ in range(args.repeats)]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in ms:
        print("%-15s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])), flush=True)
    out = {"envs": n, "steps": steps, "batch": b, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "ms": ms, "median_ms": med,
           "spread": spread, "stats": list(learner.stats()), "torch_over_device": med["torch"] / med["device"],
           "combined_spread": spread["device"] + spread["torch"], "line_gbytes_per_s": b * 128 / (med["device"] * 1e-3) / 1e9}
    print("torch / device = %.2f (the two legs' combined spread %.2f %%)" % (out["torch_over_device"], 100 * out["combined_spread"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

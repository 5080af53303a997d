"""What the rollout storage costs (include/crl.h "rollout storage"): ONE process per table, legs alternating inside every repeat, device
events around each leg, medians and spreads.

    python tools/ab/rollout_storage.py --table a [--envs 65536] [--steps 32] [--repeats 7] [--warmup 2] [--out FILE.json]
    python tools/ab/rollout_storage.py --table b [--envs 65536] [--steps 32] [--batch 262144] [--repeats 7] [--calls 5] [--out FILE.json]

Table a (per step, a light Policy at `envs` envs, `steps` steps per rollout):
  act              policy.act_rollout(obs, reset=done) alone
  act_record       ... followed by storage.record(...) and storage.outcome(...): what the storage adds per step is this minus `act`
  finish           storage.finish(last_values): GAE and the two statistics passes, per rollout
  begin            the carrying storage.begin(), per rollout
and the bytes the storage holds against a float32 FrameStackTensor copy per step of the same T and N (table c of the lab notes).
Table b (per call, `batch` samples drawn uniformly from the T * N of the storage):
  gather_f32 / gather_u8   storage.gather(idx) with every output
  torch_index_select       the torch restatement: float32 stacks [batch][4][42][42] held as they are, index_select by a permutation
                           (observations only: the scalars are noise beside 28 KB per sample)
  copy                     a device copy of the float32 output's size, for the bandwidth the machine gives a plain stream
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from competitive_rl_amd import spaces  # noqa: E402
from competitive_rl_amd.policy_serving import Policy, _random_light_weights  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402


def span(fn):
    """fn() -> the number of units it ran; device events around it -> milliseconds per unit"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    units = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / units


def plain(name, fn):
    """the measuring function of a leg that is one span"""
    return lambda: {name: span(fn)}


def timed(legs, repeats, warmup):
    """{leg: measure}, measure() -> {series: milliseconds} of one repeat (`plain`, or a function that places further events of its own).
    `warmup` unrecorded rounds, then `repeats` rounds with another leg first in every round -> every series' values, medians, spreads"""
    order = list(legs)
    for k in order:
        for _ in range(warmup):
            legs[k]()
        torch.cuda.synchronize()
        print("warmed up", k, flush=True)
    ms = {}
    for r in range(repeats):
        for k in order[r % len(order):] + order[:r % len(order)]:
            for series, v in legs[k]().items():
                ms.setdefault(series, []).append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    for k in ms:
        print("%-20s median %.4f ms  spread %.2f %%  repeats %s" % (k, med[k], 100 * spread[k], " ".join("%.4f" % x for x in ms[k])), flush=True)
    return ms, med, spread


def table_a(args, out):
    n, steps = args.envs, args.steps
    w = {**_random_light_weights(), "critic_w": (np.random.RandomState(1).standard_normal((1, 1600)) * 0.05).astype(np.float32),
         "critic_b": np.array([0.1], np.float32)}
    pol = Policy(spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3), n, use_light_model=True, weights=w)
    free0 = torch.cuda.mem_get_info()[0]
    st = RolloutStorage(steps, n)
    out["storage_bytes"], out["storage_bytes_device_delta"] = st.nbytes(), free0 - torch.cuda.mem_get_info()[0]
    out["float32_restatement_bytes"] = steps * n * (4 * 42 * 42 * 4 + 4 * 5 + 1)
    print("storage: %.3f GB held (%.3f GB less free device memory); a float32 stack per step: %.3f GB; ratio %.4f" % (
        out["storage_bytes"] / 1e9, out["storage_bytes_device_delta"] / 1e9, out["float32_restatement_bytes"] / 1e9,
        out["storage_bytes"] / out["float32_restatement_bytes"]))
    frames = [(torch.randint(0, 256, (n, 1, 42, 42), device="cuda", dtype=torch.uint8) * (torch.rand((n, 1, 42, 42), device="cuda") > 0.7)).contiguous()
              for _ in range(4)]
    done = (torch.arange(n, device="cuda") % 64 == 17).to(torch.uint8)
    acts2 = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    rew2 = torch.randn((n, 2), device="cuda")
    last = torch.randn((n,), device="cuda")
    st.begin(pol)

    def act():
        for t in range(steps):
            pol.act_rollout(frames[t % 4], reset=done, out=acts2[:, 0])
        return steps

    def act_record():
        for t in range(steps):
            f = frames[t % 4]
            values, actions, logp = pol.act_rollout(f, reset=done, out=acts2[:, 0])
            st.record(f, done, values, actions, logp)
            st.outcome(rew2[:, 0], done)
        return steps

    values, actions, logp = pol.act_rollout(frames[0], reset=done, out=acts2[:, 0])  # (what record_only stores over and over)

    def record_only():
        for t in range(steps):
            st.record(frames[t % 4], done, values, actions, logp)
            st.outcome(rew2[:, 0], done)
        return steps

    # a rollout has to be finished before the next one is carried: finish and begin run behind every recording leg, under events of
    # their own
    def recording(name, leg):
        def measure():
            per_step = span(leg)
            f0, f1, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f0.record()
            st.finish(last)
            f1.record()
            st.begin()
            b1.record()
            b1.synchronize()
            return {name: per_step, "finish": f0.elapsed_time(f1), "begin": f1.elapsed_time(b1)}
        return measure

    ms, med, spread = timed({"act": plain("act", act), "act_record": recording("act_record", act_record),
                             "record_only": recording("record_only", record_only)}, args.repeats, args.warmup)
    out["record_cost_ms"], out["record_over_act"] = med["act_record"] - med["act"], (med["act_record"] - med["act"]) / med["act"]
    moved = n * (1764 + 1776 + 27 + 14)
    out["record_only_GBps"] = moved / (med["record_only"] * 1e-3) / 1e9
    print("record + outcome beside act_rollout: %+.4f ms per step = %+.2f %% of the act call; alone %.4f ms = %.0f GB/s over %.1f MB moved" % (
        out["record_cost_ms"], 100 * out["record_over_act"], med["record_only"], out["record_only_GBps"], moved / 1e6))
    st.close(), pol.close()
    return ms, med, spread


def table_b(args, out):
    n, steps, b = args.envs, args.steps, args.batch
    st = RolloutStorage(steps, n)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    zero_f, none = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    for t in range(steps):
        obs = torch.randint(0, 256, (n, 1, 42, 42), device="cuda", dtype=torch.uint8, generator=g)
        st.record(obs, (torch.rand(n, device="cuda", generator=g) < 0.01), zero_f, None, zero_f)
        st.outcome(zero_f, none)
    st.finish()
    idx = [torch.randint(0, steps * n, (b,), device="cuda", generator=g) for _ in range(2)]
    base = torch.randint(0, 256, (b, 4, 42, 42), device="cuda", dtype=torch.uint8, generator=g).float()  # the torch restatement's storage
    perm = [torch.randperm(b, device="cuda", generator=g) for _ in range(2)]
    out_f32, out_u8 = st.empty_batch(b), st.empty_batch(b, obs_dtype=torch.uint8)
    base_out, copy_out = torch.empty_like(base), torch.empty_like(base)
    calls = args.calls

    def leg(fn):
        def run():
            for c in range(calls):
                fn(c % 2)
            return calls
        return run

    legs = {"gather_f32": leg(lambda c: st.gather(idx[c], out=out_f32)), "gather_u8": leg(lambda c: st.gather(idx[c], out=out_u8)),
            "torch_index_select": leg(lambda c: torch.index_select(base, 0, perm[c], out=base_out)), "copy": leg(lambda c: copy_out.copy_(base))}
    ms, med, spread = timed({k: plain(k, fn) for k, fn in legs.items()}, args.repeats, args.warmup)
    want = torch.index_select(base, 0, perm[0])
    assert torch.equal(torch.index_select(base, 0, perm[0], out=base_out), want)
    per = {"gather_f32": 4 * 1764 + 4 * 7056 + 8 + 40, "gather_u8": 4 * 1764 + 4 * 1764 + 8 + 40, "torch_index_select": 2 * 4 * 7056 + 8, "copy": 2 * 4 * 7056}
    for k, bytes_per in per.items():
        out[k + "_GBps"] = b * bytes_per / (med[k] * 1e-3) / 1e9
        print("%-20s %.1f GB/s over %d bytes per sample" % (k, out[k + "_GBps"], bytes_per))
    out["gather_f32_over_torch"] = med["gather_f32"] / med["torch_index_select"]
    out["traffic_ratio"] = per["gather_f32"] / per["torch_index_select"]
    both = spread["gather_f32"] + spread["torch_index_select"]
    print("gather_f32 / torch_index_select = %.4f (traffic ratio %.3f; the two legs' combined spread %.2f %%)" % (
        out["gather_f32_over_torch"], out["traffic_ratio"], 100 * both))
    st.close()
    return ms, med, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", choices=("a", "b"), required=True)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_storage.py measures on the GPU; none is visible")
    torch.manual_seed(0)
    out = {"table": args.table, "envs": args.envs, "steps": args.steps, "batch": args.batch, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    ms, med, spread = (table_a if args.table == "a" else table_b)(args, out)
    out.update({"ms": ms, "median_ms": med, "spread": spread})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

"""The bits and the refusals of both rollout storages on small fixed cases, for a parent-against-branch `diff` (a refactor of the step
counters, the GAE rule, the advantages' statistics or the normalised advantage must not move one): ONE process, one line per result,
nothing timed.  The companion of ppo_bits.py and car_bits.py, whose learners read the storages through their views.

    python tools/ab/rollout_bits.py [--only pong|car|refusals] > bits.txt

It goes through the Python interface alone, so it runs unchanged in a checkout of the parent.
  RolloutStorage     N in {1, 67, 11000} (the last: 66 000 samples, a second trip of the statistics' lanes), T = 6, recorded step by
                     step from seeded made-up frames, resets, actions, values, log-probs, rewards and dones.  Finished with and
                     without normalisation.  Lines: sha256 of `returns` and `advantages` gathered in order; stats() as hex floats;
                     sha256 of a float32 batch (every field) gathered at a seeded idx with repeats.
  CarRolloutStorage  (rows, T) in {(2, 1), (48, 6), (260, 253)} (the last: 65 780 samples), both cars, loaded as an ACTIVE rollout whose
                     steps all have their outcome -- made-up lines, every seventh sample dead --, then finished.  The same lines, and
                     sha256 of state_dict()["contents"]["lines"].
  refusals           per storage the text of each state-machine refusal: record out of turn and after the finish, outcome without a
                     record and twice, early finish, early gather, stats without normalisation, a state that does not fit -- through
                     load_state_dict and handed to the C call as it is.
Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import competitive_rl_amd as crl  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402

F = np.float32
PONG_SIZES, PONG_T = (1, 67, 11000), 6
CAR_CASES = ((2, 1), (48, 6), (260, 253))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def hexes(values):
    return " ".join(float(x).hex() for x in values)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def report(tag, st, total, fields):
    """the lines of one finished storage"""
    everything = st.gather(torch.arange(total, device="cuda"), fields=("returns", "advantages"))
    print("%s returns %s advantages %s" % (tag, sha(everything.returns), sha(everything.advantages)))
    if st.normalize_advantage:
        print("%s stats %s" % (tag, hexes(st.stats())))
    idx = dev(np.random.default_rng(total).integers(0, total, min(total + 3, 300), dtype=np.int64))
    batch = st.gather(idx, fields=fields)
    print("%s batch %s" % (tag, sha(*[t for t in batch if t is not None])), flush=True)


def record_pong(st, rs, steps):
    n = st.num_envs
    for _ in range(steps):
        frame = rs.randint(0, 256, (n, 1, 42, 42)).astype(np.uint8) * (rs.random_sample((n, 1, 42, 42)) > 0.7)
        st.record(dev(frame), dev((rs.random_sample(n) < 0.1).astype(np.uint8)), dev(rs.standard_normal(n).astype(F)),
                  dev(rs.randint(0, 3, n).astype(np.int32)), dev(-rs.random_sample(n).astype(F)))
        st.outcome(dev(rs.standard_normal(n).astype(F)), dev((rs.random_sample(n) < 0.2).astype(np.uint8)))


def run_pong():
    for n in PONG_SIZES:
        rs = np.random.RandomState(500 + n)
        st = RolloutStorage(PONG_T, n)
        st.begin(dev(rs.randint(0, 256, (n, 4, 42, 42)).astype(np.uint8)))
        record_pong(st, rs, PONG_T)
        last = dev(rs.standard_normal(n).astype(F))
        for normalize in (True, False):
            st.normalize_advantage = normalize
            st.finish(last)
            report("pong n %d normalize %d" % (n, normalize), st, PONG_T * n, None)
        st.close()


def car_lines(rows, T, seed):
    """uint32 [T * rows, 32] (include/crl.h "car rollout storage"): made-up words 0 .. 25, 20 % dones, every seventh sample dead"""
    rs = np.random.RandomState(seed)
    S = T * rows
    live = np.arange(S) % 7 != 6
    ln = np.zeros((S, 32), F)
    ln[:, :26] = rs.standard_normal((S, 26)).astype(F)
    ln[~live, :25] = 0
    out = ln.view(np.uint32)
    out[:, 28] = live.astype(np.uint32) | ((rs.random_sample(S) < 0.2).astype(np.uint32) << 1)
    return out, rs.standard_normal((rows // 2, 2)).astype(F)


def car_dict(n, T, lines, state="active", step=None, outcomes=None):
    return {"kind": "CarRolloutStorage", "num_steps": T, "num_envs": n, "players": 2, "cars": (0, 1), "gamma": 0.99, "gae_lambda": 0.95,
            "normalize_advantage": True, "state": state, "step": T if step is None else step, "outcomes": T if outcomes is None else outcomes,
            "contents": {"lines": lines, "stats": np.zeros(3), "normalized": False}}


def run_car():
    for rows, T in CAR_CASES:
        n = rows // 2
        env = crl.HipCarVecEnv(n, seed=2)
        st = crl.CarRolloutStorage(env, T, cars=(0, 1))
        lines, last = car_lines(rows, T, 700 + rows)
        st.load_state_dict(car_dict(n, T, lines))
        for normalize in (True, False):
            st.normalize_advantage = normalize
            st.finish(dev(last))
            tag = "car rows %d T %d normalize %d" % (rows, T, normalize)
            report(tag, st, T * rows, None)
            print("%s lines %s" % (tag, sha(st.state_dict()["contents"]["lines"])), flush=True)
        st.close(), env.close()


def refusal(tag, fn):
    try:
        fn()
        print("refusal %s: NOT REFUSED" % tag)
    except Exception as e:  # noqa: BLE001  (the text is the result)
        print("refusal %s: %s: %s" % (tag, type(e).__name__, e), flush=True)


def refusals_pong():
    n, T = 3, 2
    rs = np.random.RandomState(1)
    st = RolloutStorage(T, n, normalize_advantage=False)
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    misfit = (C.c_int32 * 4)(2, 2, 1, 0)  # finished with one outcome of two
    refusal("pong outcome, fresh", lambda: st.outcome(torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")))
    refusal("pong finish, fresh", st.finish)
    refusal("pong gather, fresh", lambda: st.gather(idx))
    st.begin()
    record_pong(st, rs, 1)
    refusal("pong outcome, twice", lambda: st.outcome(torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")))
    refusal("pong finish, early", st.finish)
    refusal("pong gather, early", lambda: st.gather(idx))
    refusal("pong state_dict, middle", lambda: st.state_dict(contents=False))
    mid = st.state_dict()
    record_pong(st, rs, 1)
    refusal("pong record, past the end", lambda: record_pong(st, rs, 1))
    st.finish()
    refusal("pong record, finished", lambda: record_pong(st, rs, 1))
    refusal("pong stats, not normalised", st.stats)
    refusal("pong load, misfit", lambda: st.load_state_dict(dict(mid, state="finished")))
    refusal("pong load, no contents", lambda: st.load_state_dict(dict(mid, contents=None)))
    refusal("pong set_state, misfit", lambda: st._copy_state(st._L.crl_rollout_set_state, misfit, 0, None, None, 0, {}))
    st.close()


def refusals_car():
    n, T = 3, 2
    env = crl.HipCarVecEnv(n, seed=2)
    policy = crl.CarPolicy(env, seed=0)
    rs = np.random.RandomState(1)
    policy.add_network("learner", {k: rs.uniform(-0.3, 0.3, s).astype(F) for k, s in crl.rules.CAR_POLICY_SHAPES.items()})
    policy.assign(0, "learner"), policy.assign(1, "learner")
    env.reset()
    st = crl.CarRolloutStorage(env, T, cars=(0, 1), normalize_advantage=False)
    acts, obs = torch.zeros((n, 2, 2), device="cuda"), torch.empty((n, 2, 21), device="cuda")
    values, logp = policy.act_rollout(acts, obs_out=obs)
    rew, done = torch.zeros((n, 2), device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    record = lambda t: st.record(t, policy, "learner", obs, acts, values, logp)  # noqa: E731
    misfit = (C.c_int32 * 4)(2, 2, 1, 0)
    refusal("car outcome, fresh", lambda: st.outcome(0, rew, done))
    refusal("car finish, fresh", st.finish)
    refusal("car gather, fresh", lambda: st.gather(idx))
    st.begin()
    refusal("car record, out of turn", lambda: record(1))
    record(0)
    refusal("car record, twice", lambda: record(0))
    refusal("car outcome, no record", lambda: st.outcome(1, rew, done))
    st.outcome(0, rew, done)
    refusal("car outcome, twice", lambda: st.outcome(0, rew, done))
    refusal("car finish, early", st.finish)
    refusal("car gather, early", lambda: st.gather(idx))
    refusal("car state_dict, middle", lambda: st.state_dict(contents=False))
    mid = st.state_dict()
    record(1)
    refusal("car record, past the end", lambda: record(2))
    st.outcome(1, rew, done)
    st.finish()
    refusal("car record, finished", lambda: record(0))
    refusal("car stats, not normalised", st.stats)
    refusal("car load, misfit", lambda: st.load_state_dict(dict(mid, state="finished")))
    refusal("car load, no contents", lambda: st.load_state_dict(dict(mid, contents=None)))
    refusal("car set_state, misfit", lambda: crl._native.check(st._L.crl_car_rollout_set_state(st._h, misfit, 0, None, None, st._stream())))
    st.close(), policy.close(), env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("pong", "car", "refusals"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bits.py runs on the GPU; none is visible")
    for name, fns in (("pong", (run_pong,)), ("car", (run_car,)), ("refusals", (refusals_pong, refusals_car))):
        if args.only in (None, name):
            for fn in fns:
                fn()


if __name__ == "__main__":
    main()

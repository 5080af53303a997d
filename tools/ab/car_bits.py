"""The bits of the CarRacing learner, the CarRacing league and the Pong ledger on small fixed cases, for a parent-against-branch `diff`
(a refactor of the optimiser step, the weighted draw, the PFSP fill or the booking of finished episodes must not move one): ONE process,
one line per result, nothing timed.  The companion of ppo_bits.py, which covers the two Pong learners.

    python tools/ab/car_bits.py [--only ppo|league|ledger] > bits.txt

It goes through the Python interface alone, so it runs unchanged in a checkout of the parent.
  CarPPO        the pool of tests/car_ppo_cases.py in a CarRolloutStorage, the weights perturbed by 0.1, B in its CASES with idx from a
                seeded numpy generator (repeats and dead samples included).  Lines: sha256 of grad_blob(); stats() as hex floats; sha256
                of weights, m and v of state_dict() after three grad + step pairs on three further draws of idx.
  CarLeague     n in {1, 65, 300} envs, a pool of five (three styles, two networks).  40 steps of seeded made-up rewards and done flags
                (about one env in five ends per step; returns that win, lose and tie -- every fourth reward pair is equal --, and a NaN
                reward in env 0 at step 3), pfsp_weights("hard", 2, 1) after step 20.  Lines after steps 20 and 40: sha256 of
                counters_device(), assignment(), weights() and the four tensors of env_state().
  LeagueLedger  the same n, steps and PFSP schedule over a pool of five; integer rewards in {-1, 0, 1}, the ids that update() hands back
                fed to the next step with every seventh env's id moved outside the pool (7 or -1).  Lines: sha256 of counters_device(),
                the `ignored` count, the ids, weights() and the three tensors of env_state().
Needs a GPU; there is no fallback."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import competitive_rl_amd as crl  # noqa: E402
from competitive_rl_amd.ledger import LeagueLedger  # noqa: E402
from tests import car_policy_cases as CP  # noqa: E402
from tests import car_ppo_cases as Q  # noqa: E402

SIZES, POOL, STEPS, PFSP_AT = (1, 65, 300), 5, 40, 20


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def sha_dict(d):
    return sha(*[d[k] for k in sorted(d)])


def run_ppo():
    env = crl.HipCarVecEnv(Q.N_ENVS, seed=3)
    storage = crl.CarRolloutStorage(env, Q.T, cars=(0, 1))
    po = Q.pool()
    po.fill(storage)
    weights = Q.perturbed(Q.base_weights(), 0.1)
    print("ppo pool lines %s" % sha(po.lines()), flush=True)
    for b in Q.CASES:
        rs = np.random.default_rng(1000 + b)
        idx = [torch.from_numpy(rs.integers(0, po.size, b, dtype=np.int64)).cuda() for _ in range(4)]
        learner = crl.CarPPO(weights, lr=3e-3, **Q.HYPER)
        learner.grad(storage, idx[0])
        print("ppo B %d grad %s" % (b, sha(learner.grad_blob())))
        print("ppo B %d stats %s" % (b, " ".join(float(x).hex() for x in learner.stats())))
        for k in range(1, 4):
            learner.grad(storage, idx[k])
            learner.step()
        sd = learner.state_dict()
        print("ppo B %d state steps %d weights %s m %s v %s" % (b, sd["steps"], sha_dict(sd["weights"]), sha_dict(sd["m"]), sha_dict(sd["v"])), flush=True)
        learner.close()
    storage.close(), env.close()


def made_up(n, seed):
    """rewards float32 [STEPS, n, 2] and dones uint8 [STEPS, n]"""
    rs = np.random.RandomState(seed)
    rewards = (rs.standard_normal((STEPS, n, 2)) * 3).astype(np.float32)
    rewards[:, ::4, 1] = rewards[:, ::4, 0]  # ties
    rewards[3, 0, 0] = np.nan
    dones = (rs.random_sample((STEPS, n)) < 0.2).astype(np.uint8)
    dones[5, 0] = 1  # (the NaN return is booked)
    return rewards, dones


def run_league():
    for n in SIZES:
        env = crl.HipCarVecEnv(n, seed=0, done_policy="car0")
        policy, drivers = crl.CarPolicy(env, seed=0), crl.CarDrivers(env, seed=0)
        for k, name in enumerate(("a", "b")):
            policy.add_network(name, CP.random_weights(k + 1, 2.0))
        league = crl.CarLeague(env, policy, drivers, seed=17)
        drivers.set_style("fast", "RULE_BASED", epsilon=0.1)
        for add, name in ((league.add_style, "RANDOM"), (league.add_network, "a"), (league.add_style, "RULE_BASED"), (league.add_network, "b"),
                          (league.add_style, "fast")):
            add(name)
        assert league.agents == POOL
        league.set_weights([3, 1, 0, 9, 2])
        env.reset()
        league.reset_assignment()
        rewards, dones = made_up(n, 100 + n)
        for t in range(STEPS):
            league.step(torch.from_numpy(rewards[t]).cuda(), torch.from_numpy(dones[t]).cuda())
            if t + 1 == PFSP_AT:
                league.pfsp_weights("hard", 2, 1)
            if t + 1 in (PFSP_AT, STEPS):
                print("league n %d step %d counters %s assignment %s weights %s env_state %s" % (
                    n, t + 1, sha(league.counters_device()), sha(league.assignment()), sha(league.weights()), sha(*league.env_state())), flush=True)
        league.close(), drivers.close(), policy.close(), env.close()


def run_ledger():
    for n in SIZES:
        ledger = LeagueLedger(n, POOL, "cuda", seed=23, env_id_base=2 ** 33)
        ledger.set_weights([3, 1, 0, 9, 2])
        rs = np.random.RandomState(200 + n)
        ids = torch.from_numpy(rs.randint(0, POOL, n).astype(np.int32)).cuda()
        for t in range(STEPS):
            reward = torch.from_numpy(rs.randint(-1, 2, n).astype(np.float32)).cuda()
            done = torch.from_numpy((rs.random_sample(n) < 0.2).astype(np.uint8)).cuda()
            ids = ledger.update(ids, reward, done, redraw=True)
            ids[(t % 7)::7] = 7 if t % 2 else -1  # ids outside the pool: booked as `ignored`, redrawn when their episode ends
            if t + 1 == PFSP_AT:
                ledger.pfsp_weights("hard", 2, 1)
            if t + 1 in (PFSP_AT, STEPS):
                print("ledger n %d step %d counters %s ignored %d ids %s weights %s env_state %s" % (
                    n, t + 1, sha(ledger.counters_device()), ledger.counters()["ignored"], sha(ids), sha(ledger.weights()), sha(*ledger.env_state())),
                    flush=True)
        ledger.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("ppo", "league", "ledger"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("car_bits.py runs on the GPU; none is visible")
    for name, fn in (("ppo", run_ppo), ("league", run_league), ("ledger", run_ledger)):
        if args.only in (None, name):
            fn()


if __name__ == "__main__":
    main()

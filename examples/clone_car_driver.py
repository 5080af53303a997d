"""Clone the RULE_BASED CarRacing driver into the car policy's MLP(21, 2) by DAgger, the whole loop on the device
(competitive_rl_amd/car_learner.py, include/crl.h "car ppo update, teacher targets"):

    act_rollout -> rule.act(target[t]) -> record -> step_device(render=False) -> outcome -> finish -> update(teacher=...) -> push

The LEARNER's sampling net drives both cars, so the states are the ones the clone itself reaches; a second ``CarDrivers`` with
RULE_BASED (epsilon 0) on both cars answers every visited state into ``target[t]`` of a scratch (T, N, 2, 2) tensor, and the update
minimises ``0.5 |mean - target|^2`` alone: ``CarTeacher(target, loss="mse", policy_term=False)``.  The value head learns the returns
of the cloning drive meanwhile.  No pixels are drawn and nothing synchronises with the host inside an iteration; the host reads per
iteration are the lines this script prints: the learner's teacher statistics and the share of their track the cars have visited
(feature 5 of the observation, averaged over the live cars at the end of the rollout).

    python examples/clone_car_driver.py --envs 2048 --steps 64 --iterations 30
    python examples/clone_car_driver.py --baselines          # also: RULE_BASED itself and the offline clone in the same envs and steps
    python examples/clone_car_driver.py --then-league -- --iterations 40   # then examples/train_car_league.py from the clone
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import competitive_rl_amd as crl  # noqa: E402
from examples.train_car_ppo import initial_weights  # noqa: E402

OFFLINE_CLONE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "car_policy_clone.npz")


def visited_share(obs):
    live = obs.abs().sum(dim=2) > 0
    return float((obs[:, :, 5] * live).sum() / live.sum().clamp(min=1))


def baseline(a, who):
    """The visited share after every ``a.steps`` steps of a fresh env of the same seed driven by RULE_BASED itself (``who`` None) or by
    the deterministic network ``who``"""
    env = crl.HipCarVecEnv(a.envs, seed=a.seed, done_policy="car0")
    policy = crl.CarPolicy(env, seed=a.seed)
    actions = torch.zeros((a.envs, 2, 2), device=env.device)
    obs = torch.empty((a.envs, 2, 21), device=env.device)
    drivers = None
    if who is None:
        drivers = crl.CarDrivers(env, seed=a.seed)
        drivers.assign(0, "RULE_BASED"), drivers.assign(1, "RULE_BASED")
        policy.add_network("observer", initial_weights(a.seed), deterministic=True)  # (serves nobody: act_rollout only fills obs)
    else:
        policy.add_network("driver", who, deterministic=True)
        policy.assign(0, "driver"), policy.assign(1, "driver")
    env.reset()
    shares = []
    for _ in range(a.iterations):
        for _ in range(a.steps):
            if drivers is not None:
                drivers.act(actions)
            policy.act_rollout(actions, obs_out=obs)
            env.step_device(actions, render=False)
        policy.act_rollout(actions, obs_out=obs)
        shares.append(visited_share(obs))
    if drivers is not None:
        drivers.close()
    policy.close(), env.close()
    return shares


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64, help="steps per rollout")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--baselines", action="store_true", help="also drive the same envs and steps with RULE_BASED and with the offline clone")
    ap.add_argument("--then-league", action="store_true", help="hand the clone to the loop of examples/train_car_league.py")
    ap.add_argument("league_args", nargs="*", help="behind --: the command line of train_car_league.py")
    a = ap.parse_args()

    env = crl.HipCarVecEnv(a.envs, seed=a.seed, done_policy="car0")
    learner = crl.CarPPO(initial_weights(a.seed), lr=a.lr)
    policy = crl.CarPolicy(env, seed=a.seed)
    policy.add_network("learner", learner.weights())
    policy.assign(0, "learner"), policy.assign(1, "learner")
    rule = crl.CarDrivers(env, seed=a.seed)
    rule.set_style("RULE_BASED", epsilon=0.0)
    rule.assign(0, "RULE_BASED"), rule.assign(1, "RULE_BASED")
    storage = crl.CarRolloutStorage(env, a.steps, cars=(0, 1))
    actions = torch.zeros((a.envs, 2, 2), device=env.device)
    obs = torch.empty((a.envs, 2, 21), device=env.device)
    target = torch.zeros((a.steps, a.envs, 2, 2), device=env.device)
    teacher = crl.CarTeacher(target, loss="mse", policy_term=False)
    env.reset()
    values, log_probs = policy.act_rollout(actions, obs_out=obs)
    shares = []
    for it in range(a.iterations):
        t0 = time.perf_counter()
        storage.begin()
        for t in range(a.steps):
            rule.act(target[t])  # what RULE_BASED would do where the learner is
            storage.record(t, policy, "learner", obs, actions, values, log_probs)
            _, rewards, done = env.step_device(actions, render=False)
            storage.outcome(t, rewards, done)
            values, log_probs = policy.act_rollout(actions, obs_out=obs)
        storage.finish(values)
        learner.update(storage, a.epochs, a.minibatches, teacher=teacher)
        learner.push(policy, "learner")
        shares.append(visited_share(obs))  # (the iteration's host reads from here on)
        s, ts = learner.stats(), learner.teacher_stats()
        print("iteration %3d  visited share %.4f  mse term %.5f  |mean - target| %.4f  taught %.3f  value %.4f  live %d  %.1f ms" % (
            it, shares[-1], ts.term, ts.abs_err, ts.taught, s.value_loss, s.live, (time.perf_counter() - t0) * 1e3))
    clone = learner.weights()
    learner.close(), storage.close(), rule.close(), policy.close(), env.close()
    if a.baselines:
        import numpy as np

        lines = {"DAgger clone (sampling, while it learns)": shares, "RULE_BASED": baseline(a, None),
                 "offline clone (deterministic)": baseline(a, dict(np.load(OFFLINE_CLONE))), "DAgger clone (deterministic, final)": baseline(a, clone)}
        for name, v in lines.items():
            print("%-40s %s" % (name, " ".join("%.4f" % x for x in v)))
    if a.then_league:
        from examples.train_car_league import main as league_main

        league_main(["--envs", str(a.envs), "--seed", str(a.seed)] + list(a.league_args), weights=clone)


if __name__ == "__main__":
    main()

"""Train the car policy's MLP(21, 2) with PPO against a league, the whole loop on the device: the loop of train_car_ppo.py with a
``CarLeague`` (competitive_rl_amd/car_league.py) that gives car 1 of every env an opponent of its own -- RANDOM, RULE_BASED or a
snapshot of the learner -- books every race and draws harder opponents more often (PFSP):

    act_rollout -> record -> step_device(render=False) -> league.step -> outcome -> ... -> finish -> update -> push -> pfsp_weights

Every --snapshot-every iterations the learner's weights go into the next snapshot slot in ring order (``learner.push``, a device copy)
and that agent's record starts over (``league.reset_agent``).  Nothing synchronises with the host inside an iteration; the one host
read per iteration is the line this script prints, and every --report iterations the per-agent table.

    python examples/train_car_league.py --envs 1024 --steps 64 --iterations 40

The learner starts from ``initial_weights``; ``examples/clone_car_driver.py --then-league`` runs this loop from a RULE_BASED clone.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import competitive_rl_amd as crl  # noqa: E402
from examples.train_car_ppo import initial_weights  # noqa: E402


def report(league):
    c = league.counters()  # (synchronises)
    w = league.weights()
    for a, name in enumerate(league.agent_names()):
        print("    %-12s episodes %6d  win rate %5.3f  mean return %+8.2f  opponent's %+8.2f  mean length %6.1f  weight %5d" % (
            name, c["episodes"][a], c["win_rate"][a], c["mean_return"][a], c["mean_opponent_return"][a],
            c["length_sum"][a] / max(int(c["episodes"][a]), 1), w[a]))


def main(argv=None, weights=None):
    """``weights``: the learner's starting weights in place of ``initial_weights`` (examples/clone_car_driver.py --then-league hands its
    RULE_BASED clone over here); ``argv``: the command line in place of the process's."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64, help="steps per rollout")
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--snapshots", type=int, default=4, help="snapshot slots in the pool (at most 7)")
    ap.add_argument("--snapshot-every", type=int, default=5, help="iterations between snapshots")
    ap.add_argument("--report", type=int, default=5, help="iterations between per-agent tables")
    ap.add_argument("--start-elapsed", type=int, default=0,
                    help="start the envs' TimeLimit counters staggered over [this, 1000): episodes end from the first iterations on")
    a = ap.parse_args(argv)
    assert 1 <= a.snapshots <= 7

    env = crl.HipCarVecEnv(a.envs, seed=a.seed, done_policy="car0")
    learner = crl.CarPPO(initial_weights(a.seed) if weights is None else weights, lr=a.lr)
    policy = crl.CarPolicy(env, seed=a.seed)
    drivers = crl.CarDrivers(env, seed=a.seed)
    policy.add_network("learner", learner.weights())
    snapshots = ["snapshot%d" % k for k in range(a.snapshots)]
    for name in snapshots:
        policy.add_network(name, learner.weights())
    policy.assign(0, "learner")
    league = crl.CarLeague(env, policy, drivers, seed=a.seed)
    league.add_style("RANDOM"), league.add_style("RULE_BASED")
    for name in snapshots:
        league.add_network(name)
    storage = crl.CarRolloutStorage(env, a.steps, cars=(0,))
    actions = torch.zeros((a.envs, 2, 2), device=env.device)
    obs = torch.empty((a.envs, 2, 21), device=env.device)
    reward_sum = torch.zeros((), device=env.device)
    env.reset()
    if a.start_elapsed:
        st = env.get_state()
        st["elapsed"][:] = a.start_elapsed + (np.arange(a.envs) * (1000 - a.start_elapsed)) // a.envs
        env.set_state(st)
    league.reset_assignment()
    drivers.act(actions)
    values, log_probs = policy.act_rollout(actions, obs_out=obs)
    taken = 0
    for it in range(a.iterations):
        t0 = time.perf_counter()
        reward_sum.zero_()
        storage.begin()
        for t in range(a.steps):
            storage.record(t, policy, "learner", obs, actions, values, log_probs)
            _, rewards, done = env.step_device(actions, render=False)
            league.step(rewards, done)  # books the finished races; their envs' car 1 has its next driver from here on
            storage.outcome(t, rewards, done)
            reward_sum += rewards[:, 0].mean()
            drivers.act(actions)
            values, log_probs = policy.act_rollout(actions, obs_out=obs)
        storage.finish(values)
        learner.update(storage, a.epochs, a.minibatches)
        learner.push(policy, "learner")
        if (it + 1) % a.snapshot_every == 0:
            name = snapshots[taken % len(snapshots)]
            learner.push(policy, name)
            league.reset_agent(name)
            taken += 1
        league.pfsp_weights("hard", 2, 1)
        s = learner.stats()  # (the iteration's host read)
        print("iteration %3d  mean step reward %+.4f  policy %+.4f  value %.4f  kl %+.5f  clipped %.3f  live %d  snapshots %d  %.1f ms" % (
            it, float(reward_sum) / a.steps, s.policy_loss, s.value_loss, s.approx_kl, s.clip_fraction, s.live, taken, (time.perf_counter() - t0) * 1e3))
        if (it + 1) % a.report == 0 or it + 1 == a.iterations:
            report(league)
    league.close(), learner.close(), storage.close(), drivers.close(), policy.close(), env.close()


if __name__ == "__main__":
    main()

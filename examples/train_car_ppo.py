"""Train the car policy's MLP(21, 2) with PPO, the whole loop on the device (competitive_rl_amd/car_learner.py):

    act_rollout -> record -> step_device(render=False) -> outcome -> finish -> update -> push

No pixels are drawn and nothing synchronises with the host inside an iteration; the one host read per iteration is the line this
script prints: the share of their track that the cars have visited (feature 5 of the observation, averaged over the live cars at the
end of the rollout), the mean step reward and the learner's statistics.

    python examples/train_car_ppo.py --envs 1024 --steps 64 --iterations 40
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import competitive_rl_amd as crl  # noqa: E402


def initial_weights(seed):
    """torch's default initialisation of MLP(21, 2) (uniform +- 1 / sqrt(fan_in)), a small policy head and log_std = -0.5"""
    rs = np.random.RandomState(seed)
    u = lambda shape, fan, scale=1.0: (rs.uniform(-1, 1, shape) * scale / np.sqrt(fan)).astype(np.float32)  # noqa: E731
    return dict(fc1_w=u((100, 21), 21), fc1_b=u((100,), 21), policy_w=u((2, 100), 100, 0.1), policy_b=np.array([0.0, 0.3], np.float32),
                value_w=u((1, 100), 100), value_b=np.zeros(1, np.float32), log_std=np.full(2, -0.5, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64, help="steps per rollout")
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    env = crl.HipCarVecEnv(a.envs, seed=a.seed, done_policy="car0")
    learner = crl.CarPPO(initial_weights(a.seed), lr=a.lr)
    policy = crl.CarPolicy(env, seed=a.seed)
    policy.add_network("learner", learner.weights())
    policy.assign(0, "learner"), policy.assign(1, "learner")
    storage = crl.CarRolloutStorage(env, a.steps, cars=(0, 1))
    actions = torch.zeros((a.envs, 2, 2), device=env.device)
    obs = torch.empty((a.envs, 2, 21), device=env.device)
    reward_sum = torch.zeros((), device=env.device)
    env.reset()
    values, log_probs = policy.act_rollout(actions, obs_out=obs)
    for it in range(a.iterations):
        t0 = time.perf_counter()
        reward_sum.zero_()
        storage.begin()
        for t in range(a.steps):
            storage.record(t, policy, "learner", obs, actions, values, log_probs)
            _, rewards, done = env.step_device(actions, render=False)
            storage.outcome(t, rewards, done)
            reward_sum += rewards.mean()
            values, log_probs = policy.act_rollout(actions, obs_out=obs)
        storage.finish(values)
        learner.update(storage, a.epochs, a.minibatches)
        learner.push(policy, "learner")
        live = obs.abs().sum(dim=2) > 0
        visited = float((obs[:, :, 5] * live).sum() / live.sum().clamp(min=1))  # (the iteration's one host read)
        s = learner.stats()
        print("iteration %3d  visited share %.4f  mean step reward %+.4f  policy %+.4f  value %.4f  kl %+.5f  clipped %.3f  live %d  %.1f ms" % (
            it, visited, float(reward_sum) / a.steps, s.policy_loss, s.value_loss, s.approx_kl, s.clip_fraction, s.live, (time.perf_counter() - t0) * 1e3))
    learner.close(), storage.close(), policy.close(), env.close()


if __name__ == "__main__":
    main()

"""A DAgger step of the CarRacing learner on the device: the loop of tests/test_hip_car_learner_loop.py (16 envs x 2 cars, the learner's
sampling net drives both) with T = 4 and a second ``CarDrivers`` -- RULE_BASED, epsilon 0, assigned to both cars -- that writes what
RULE_BASED would do in each visited state into ``target[t]`` of a scratch (T, N, 2, 2) tensor.  The recorded targets equal
rules.car_driver_reference on the env's own state bit for bit; the teacher gradient of the first minibatch equals
rules.car_ppo_teacher_loss_reference fed ``gather``'s own output and the recorded targets, within the budget rule of
tests/car_ppo_cases.py."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from competitive_rl_amd import rules as R  # noqa: E402
from tests import car_policy_cases as CP  # noqa: E402
from tests import car_ppo_cases as Q  # noqa: E402
from tests.test_hip_car_drivers import Tracks, _need_gpu, bits, reference  # noqa: E402

N, T = 16, 4
HYPER = dict(Q.HYPER, lr=3e-3)
SEED = 7


def build():
    import competitive_rl_amd as crl

    o = types.SimpleNamespace()
    o.env = crl.HipCarVecEnv(N, seed=SEED, done_policy="car0")
    o.policy = crl.CarPolicy(o.env, seed=SEED + 1)
    w = CP.random_weights(SEED, 2.0)
    o.policy.add_network("learner", w)
    o.policy.assign(0, "learner"), o.policy.assign(1, "learner")
    o.rule = crl.CarDrivers(o.env, seed=SEED + 2)
    o.rule.assign(0, "RULE_BASED"), o.rule.assign(1, "RULE_BASED")
    o.storage = crl.CarRolloutStorage(o.env, T, cars=(0, 1))
    o.learner = crl.CarPPO(w, **HYPER)
    o.env.reset()
    st = o.env.get_state()
    st["elapsed"][::3] = 1000 - 2  # auto-resets inside the rollout: a new track under the same teacher
    o.env.set_state(st)
    o.acts = torch.zeros((N, 2, 2), device="cuda")
    o.obs = torch.zeros((N, 2, 21), device="cuda")
    o.target = torch.full((T, N, 2, 2), float("nan"), device="cuda")
    return o


def test_recorded_targets_are_the_rule_and_the_teacher_gradient_is_the_reference():
    _need_gpu()
    import competitive_rl_amd as crl

    o = build()
    tracks = Tracks(o.env)
    styles, assign = {1: R.check_car_style()}, np.ones((N, 2), np.int32)
    want = np.zeros((T, N, 2, 2), np.float32)
    o.storage.begin()
    values, logp = o.policy.act_rollout(o.acts, obs_out=o.obs)
    resets = 0
    for t in range(T):
        o.rule.act(o.target[t])  # the teacher's answer to the state the learner's action is about to leave
        state = o.env.get_state()
        tracks.refresh(state)
        want[t] = reference(state, tracks, styles, assign, SEED + 2, np.arange(N), t)
        o.storage.record(t, o.policy, "learner", o.obs, o.acts, values, logp)
        _, rew, done = o.env.step_device(o.acts, render=False)
        resets += int(done.sum())
        o.storage.outcome(t, rew, done)
        values, logp = o.policy.act_rollout(o.acts, obs_out=o.obs)
    o.storage.finish(values)
    got = o.target.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).all() and resets >= N // 3
    assert np.abs(got).max() <= 1.0 and len(np.unique(got)) > N

    total = T * N * 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED)
    first = torch.randperm(total, device="cuda", generator=gen)[:total // 2]
    b = o.storage.gather(first)
    args = [t.cpu().numpy() for t in (b.obs, b.actions, b.old_log_probs, b.returns, b.advantages, b.live)]
    rows = got.reshape(total, 2)[first.cpu().numpy()]
    w = o.learner.weights()
    for kw in (dict(loss="mse", policy_term=False), dict(loss="ce", coef=0.3)):
        teacher = crl.CarTeacher(o.target, **kw)
        o.learner.grad(o.storage, first, teacher=teacher)
        blob = o.learner.grad_blob().cpu().numpy().copy()
        stats, tstats = o.learner.stats(), o.learner.teacher_stats()
        rule = dict(target=rows, log_std=None, loss=kw["loss"], coef=kw.get("coef", 1.0), policy_term=int(kw.get("policy_term", True)))
        r64 = R.car_ppo_teacher_loss_reference(w, *args, HYPER, teacher=rule)
        order = np.arange(len(rows))[::-1].copy()
        refs = [R.car_ppo_teacher_loss_reference(w, *args, HYPER, torch.float32, teacher=rule),
                R.car_ppo_teacher_loss_reference(w, *[a[order] for a in args], HYPER, torch.float32, teacher=dict(rule, target=rows[order]))]
        e_ref = {k: max(Q.rel_err(r["grads"], r64["grads"])[k] for r in refs) for k in Q.KEYS}
        budget = {k: max(Q.FACTOR * e_ref[k], 2 * Q.ULP1) for k in Q.KEYS}  # the rule of tests/car_ppo_cases.py
        err = Q.rel_err(R.car_policy_unpack(blob), r64["grads"])
        print("teacher loop %s, first minibatch of %d (L %d): error / budget %s" % (kw["loss"], len(rows), stats.live,
                                                                                  {k: "%.2f" % (err[k] / budget[k]) for k in Q.KEYS}))
        assert stats.live == r64["live"] and 0 < stats.live <= len(rows) and tstats.taught == r64["taught"] == 1.0
        for k in Q.KEYS:
            assert err[k] <= budget[k], (kw, k, err[k], budget[k])
        top = max(1.0, float(np.abs(r64["mean"]).max()), float(np.abs(r64["logp"][args[-1] != 0]).max()))
        for k, x in zip(("term", "kl_teacher", "abs_err"), tstats[:3]):
            e = max(abs(r[k] - r64[k]) for r in refs)
            assert abs(x - r64[k]) <= max(Q.FACTOR * e, 2 * float(np.spacing(np.float32(top)))), (kw, k, x, r64[k])
    o.learner.update(o.storage, 1, 2, gen, teacher=crl.CarTeacher(o.target, loss="mse", policy_term=False))
    assert o.learner.stats().steps == 2 and o.learner.teacher_stats().taught == 1.0
    o.learner.close(), o.storage.close(), o.rule.close(), o.policy.close(), o.env.close()

"""The whole CarRacing learner loop on the device: 16 envs x 2 cars, T = 8, two iterations of act_rollout / record / step_device(render=
False) / outcome / finish / update(2 epochs, 2 minibatches) / push.  The gradient of the first minibatch against
rules.car_ppo_loss_reference fed ``gather``'s own output; resume: everything saved after iteration 1 and rebuilt in fresh objects gives
iteration 2 the bytes of the uninterrupted run; side stream: the same loop on a held side stream (tests/stream_cases.py) equals, bit
for bit, the default stream with a synchronisation after every call."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from competitive_rl_amd import rules as R  # noqa: E402
from tests import car_policy_cases as CP  # noqa: E402
from tests import car_ppo_cases as Q  # noqa: E402
from tests.test_hip_car_drivers import _need_gpu, bits  # noqa: E402

N, T, EPOCHS, BATCHES = 16, 8, 2, 2
HYPER = dict(Q.HYPER, lr=3e-3)


def build(seed=7, early=True):
    import competitive_rl_amd as crl

    o = types.SimpleNamespace()
    o.env = crl.HipCarVecEnv(N, seed=seed, done_policy="car0")
    o.policy = crl.CarPolicy(o.env, seed=seed + 1)
    w = CP.random_weights(seed, 2.0)
    o.policy.add_network("learner", w)
    o.policy.assign(0, "learner"), o.policy.assign(1, "learner")
    o.storage = crl.CarRolloutStorage(o.env, T, cars=(0, 1))
    o.learner = crl.CarPPO(w, **HYPER)
    o.gen = torch.Generator(device="cuda")
    o.gen.manual_seed(seed)
    o.env.reset()
    st = o.env.get_state()
    if early:
        st["elapsed"][::3] = 1000 - 5  # auto-resets inside both iterations
    st["elapsed"][1::3] = 1000 - T - 3  # ... and these inside the second one only
    o.env.set_state(st)
    o.acts = torch.zeros((N, 2, 2), device="cuda")
    o.obs = torch.zeros((N, 2, 21), device="cuda")
    return o


def close(o):
    o.learner.close(), o.storage.close(), o.policy.close(), o.env.close()


def rollout(o, call=lambda name, fn, *a, **kw: fn(*a, **kw), keep=lambda name, t: None):
    """begin, the opening act, T x (record, step, outcome, act), finish"""
    call("begin", o.storage.begin)
    values, logp = call("act_rollout", o.policy.act_rollout, o.acts, obs_out=o.obs)
    for t in range(T):
        for name, x in (("actions", o.acts), ("values", values), ("logp", logp)):
            keep("step%d.%s" % (t, name), x)
        call("record", o.storage.record, t, o.policy, "learner", o.obs, o.acts, values, logp)
        _, rew, done = call("step_device", o.env.step_device, o.acts, render=False)
        keep("step%d.rew" % t, rew), keep("step%d.done" % t, done)
        call("outcome", o.storage.outcome, t, rew, done)
        values, logp = call("act_rollout", o.policy.act_rollout, o.acts, obs_out=o.obs)
    call("finish", o.storage.finish, values)


def iteration(o):
    """one iteration; returns the bytes it left behind"""
    rollout(o)
    batch = o.storage.gather(torch.arange(T * N * 2, device="cuda"))
    o.learner.update(o.storage, EPOCHS, BATCHES, o.gen)
    o.learner.push(o.policy, "learner")
    out = [t.cpu().numpy().tobytes() for t in batch]
    out += [o.learner._blob().tobytes(), o.policy._blob(0)[0].tobytes(), np.asarray(o.env.get_state()).tobytes(), repr(o.storage.stats()).encode()]
    return out


def test_first_minibatch_gradient_is_the_reference_fed_the_gathers_own_output():
    _need_gpu()
    o = build()
    rollout(o)
    size = T * N * 2 // BATCHES
    first = torch.randperm(T * N * 2, device="cuda", generator=o.gen)[:size]
    o.learner.grad(o.storage, first)
    blob = o.learner.grad_blob().cpu().numpy().copy()
    stats = o.learner.stats()
    b = o.storage.gather(first)
    args = [t.cpu().numpy() for t in (b.obs, b.actions, b.old_log_probs, b.returns, b.advantages, b.live)]
    w = o.learner.weights()
    r64 = R.car_ppo_loss_reference(w, *args, HYPER)
    order = np.arange(size)[::-1].copy()
    refs = [R.car_ppo_loss_reference(w, *args, HYPER, torch.float32), R.car_ppo_loss_reference(w, *[a[order] for a in args], HYPER, torch.float32)]
    e_ref = {k: max(Q.rel_err(r["grads"], r64["grads"])[k] for r in refs) for k in Q.KEYS}
    budget = {k: max(Q.FACTOR * e_ref[k], 2 * Q.ULP1) for k in Q.KEYS}  # the rule of tests/car_ppo_cases.py
    err = Q.rel_err(R.car_policy_unpack(blob), r64["grads"])
    print("loop, first minibatch of %d (L %d): error / budget %s" % (size, stats.live, {k: "%.2f" % (err[k] / budget[k]) for k in Q.KEYS}))
    assert stats.live == r64["live"] == int(args[-1].sum()) and 0 < stats.live <= size
    for k in Q.KEYS:
        assert err[k] <= budget[k], (k, err[k], budget[k])
    # the closing act call served the same weights that recorded the samples: r is 1 within float32 rounding
    assert np.abs(r64["ratio"][args[-1] != 0] - 1).max() <= 32 * float(np.spacing(np.float32(max(1.0, np.abs(args[2]).max()))))
    close(o)


def test_resume_after_iteration_one_gives_the_bytes_of_the_uninterrupted_run():
    _need_gpu()
    import competitive_rl_amd as crl

    # (the env's state dict does not hold the TRACKS, which are a function of (seed, env id, episode): the checkpoint is taken while
    # every env is on its first episode, and the resumed env has the seed; the auto-resets fall into iteration 2)
    a = build(early=False)
    first = iteration(a)
    a_episode_1 = a.env.get_state()["episode"].copy()
    want = iteration(a)
    assert (a.env.get_state()["episode"] > a_episode_1).sum() >= N // 3  # (episodes ended inside iteration 2)
    assert first != want and a.learner.stats().steps == 2 * EPOCHS * BATCHES
    close(a)
    b = build(early=False)
    assert iteration(b) == first
    assert (b.env.get_state()["episode"] == a_episode_1).all()
    saved = dict(env=b.env.state_dict(), policy=b.policy.state_dict(), storage=b.storage.state_dict(contents=False), learner=b.learner.state_dict(),
                 gen=b.gen.get_state().clone())
    close(b)
    c = types.SimpleNamespace()
    c.env = crl.HipCarVecEnv(N, seed=7, done_policy="car0")
    c.policy = crl.CarPolicy(c.env, seed=0)
    c.storage = crl.CarRolloutStorage(c.env, T, cars=(0, 1))
    c.learner = crl.CarPPO(CP.random_weights(50))
    c.gen = torch.Generator(device="cuda")
    c.env.reset()
    c.env.load_state_dict(saved["env"]), c.policy.load_state_dict(saved["policy"]), c.storage.load_state_dict(saved["storage"])
    c.learner.load_state_dict(saved["learner"]), c.gen.set_state(saved["gen"])
    assert c.learner.hyper == dict(R.CAR_PPO_DEFAULTS, **HYPER)
    c.acts, c.obs = torch.zeros((N, 2, 2), device="cuda"), torch.zeros((N, 2, 21), device="cuda")
    got = iteration(c)
    names = ("obs", "actions", "old_log_probs", "values", "returns", "advantages", "live", "master blob", "served blob", "env state", "statistics")
    assert [n for n, x, y in zip(names, got, want) if x != y] == []
    close(c)


class CarLearnerCase:
    """The loop of this module as a chain of tests/stream_cases.py: a pass is one iteration.  Calls: begin; act_rollout; T x (record,
    step_device(render=False), outcome, act_rollout); finish; gather; update(2, 2, generator) [randperm, grad, step]; grad of a fixed
    batch (kept) and step; push.  ``reset()``, ``add_network`` and ``assign`` stay in front of the chain."""
    name = "car-learner"

    def build(self):
        o = build(seed=17)
        o.all = torch.arange(T * N * 2, device="cuda")
        o.some = torch.from_numpy(np.random.RandomState(0).randint(0, T * N * 2, 100).astype(np.int64)).cuda()
        return o

    def chain(self, rec, o, k):
        o.gen.manual_seed(300 + k)
        with rec.on("A"):
            rollout(o, rec.call, rec.keep)
            batch = rec.call("gather", o.storage.gather, o.all)
            for f, t in zip(batch._fields, batch):
                rec.keep("all." + f, t)
            rec.call("update", o.learner.update, o.storage, EPOCHS, BATCHES, o.gen)
            for key, g in sorted(rec.call("grad", o.learner.grad, o.storage, o.some).items()):
                rec.keep("grad." + key, g)
            rec.call("step", o.learner.step)
            rec.call("push", o.learner.push, o.policy, "learner")

    def finish(self, rec, o):
        rec.out["master"] = o.learner._blob()
        rec.out["served"] = o.policy._blob(0)[0]
        rec.out["env_state"] = o.env.get_state()
        rec.out["ppo_stats"] = np.array(tuple(o.learner.stats()), np.float64)
        rec.out["rollout_stats"] = np.array(o.storage.stats(), np.float64)

    def close(self, o):
        close(o)


def test_the_loop_on_a_held_side_stream_equals_the_default_stream():
    _need_gpu()
    from tests import stream_cases as SC

    case = CarLearnerCase()
    ref = SC.reference_run(case)
    side = SC.held_run(case, {"A": SC.pick_streams(1)[0]})
    assert SC.same(ref.out, side.out) == []
    dones = [ref.out["%d:step%d.done" % (k, t)] for k in range(2) for t in range(T)]
    assert sum(int(d.sum()) for d in dones) >= 6  # (episodes ended inside the chain)
    assert not np.array_equal(bits(ref.out["master"]), bits(R.car_policy_pack(CP.random_weights(17, 2.0))))
    assert np.array_equal(bits(ref.out["master"]), bits(ref.out["served"]))

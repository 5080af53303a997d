"""The CarRacing learner's PPO update on the device (include/crl.h "car ppo update"; csrc/car_ppo.hip) against float64 autograd of the
written rule (rules.car_ppo_loss_reference) within the CPU-derived budget of tests/car_ppo_cases.py, per tensor and per statistic;
two runs give the same bits; ``step()`` against rules.adam_reference bit for bit given the device's gradient and norm; the derived std
floats, the pad and the moments behind them; ``push`` into a served CarPolicy.

Measured on an MI355X (device error / budget, the largest over the tensors): see docs/LAB_NOTES_car_ppo.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from competitive_rl_amd import rules as R  # noqa: E402
from tests import car_ppo_cases as Q  # noqa: E402
from tests.test_hip_car_drivers import Tracks, _need_gpu, bits  # noqa: E402

F = np.float32
_made = {}


def filled():
    """(env, storage): the pool of car_ppo_cases in a CarRolloutStorage -- once per process, read-only"""
    if not _made:
        import competitive_rl_amd as crl

        env = crl.HipCarVecEnv(Q.N_ENVS, seed=3)
        storage = crl.CarRolloutStorage(env, Q.T, cars=(0, 1))
        Q.pool().fill(storage)
        _made.update(env=env, storage=storage)
    return _made["env"], _made["storage"]


def batch_of(which):
    return {"big": Q.big, "big_tail": Q.big_tail, "dead": Q.dead}[which]() if isinstance(which, str) else Q.chosen()[2][which]


def test_the_filled_storage_hands_out_the_pool():
    _need_gpu()
    _, storage = filled()
    po = Q.pool()
    got = storage.gather(torch.arange(po.size, device="cuda"))
    for t, want in ((got.obs, po.obs), (got.actions, po.u), (got.old_log_probs, po.logp), (got.values, po.values), (got.returns, po.ret),
                    (got.advantages, po.adv)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(want))
    assert np.array_equal(got.live.cpu().numpy().astype(bool), po.live)
    assert storage.stats() == (po.mean, po.std, int(po.live.sum()))


@pytest.mark.parametrize("which", list(Q.CASES) + ["big", "big_tail", "dead"])
def test_gradient_and_statistics_within_the_budget_and_the_same_bits_twice(which):
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, _ = Q.chosen()
    bt = batch_of(which)
    learner = crl.CarPPO(w, **Q.HYPER)
    idx = torch.from_numpy(bt.idx.astype(np.int64)).cuda()
    views = learner.grad(storage, idx)
    blob = learner.grad_blob().cpu().numpy().copy()
    stats = learner.stats()
    assert all(np.array_equal(bits(views[k].cpu().numpy()), bits(R.car_policy_unpack(blob)[k])) for k in Q.KEYS)
    learner.grad(storage, idx)
    again = learner.grad_blob().cpu().numpy()
    assert np.array_equal(bits(blob), bits(again)) and learner.stats() == stats
    assert not blob[2505:].any() and np.isfinite(blob).all()
    got = R.car_policy_unpack(blob)
    assert stats.live == bt.L and stats.steps == 0
    if bt.L == 0:
        assert not blob.any() and tuple(stats[:6]) == (0.0,) * 6
        learner.close()
        return
    err = Q.rel_err(got, bt.r64["grads"])
    print("car ppo b %s L %d: error / budget %s" % (which, bt.L, {k: "%.2f" % (err[k] / bt.budget[k]) for k in Q.KEYS}))
    for k in Q.KEYS:
        assert err[k] <= bt.budget[k], (which, k, err[k], bt.budget[k], bt.e_ref[k])
    mine = dict(zip(Q.STAT_KEYS, stats[:5]))
    serr = {k: abs(mine[k] - bt.r64[k]) for k in Q.STAT_KEYS}
    print("   statistics error / budget %s" % {k: "%.2f" % (serr[k] / bt.stat_budget[k]) for k in Q.STAT_KEYS})
    for k in Q.STAT_KEYS:
        assert serr[k] <= bt.stat_budget[k], (which, k, serr[k], bt.stat_budget[k])
    norm = float(np.sqrt((blob.astype(np.float64) ** 2).sum()))
    assert abs(stats.grad_norm - norm) <= 1e-12 * max(norm, 1.0)
    learner.close()


def test_step_is_the_adam_rule_bit_for_bit_and_the_std_floats_follow():
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, batches = Q.chosen()
    hyper = dict(Q.HYPER, lr=1e-2, max_grad_norm=0.05)  # (a step that moves log_std visibly, and a norm that clips)
    learner = crl.CarPPO(w, **hyper)
    clipped = 0
    for t, b in enumerate((130, 65, 7), start=1):
        idx = torch.from_numpy(batches[b].idx.astype(np.int64)).cuda()
        learner.grad(storage, idx)
        g = learner.grad_blob().cpu().numpy().copy()
        norm = learner.stats().grad_norm
        clipped += norm > hyper["max_grad_norm"]
        (p0, m0, v0), steps = learner._get_state()
        assert steps == t - 1
        learner.step()
        (p1, m1, v1), steps = learner._get_state()
        assert steps == t
        wp, wm, wv = R.adam_reference(p0[:2505], m0[:2505], v0[:2505], g[:2505], norm, t, hyper)
        for got, want, what in ((p1, wp, "weights"), (m1, wm, "m"), (v1, wv, "v")):
            assert np.array_equal(bits(got[:2505]), bits(want)), (t, what)
        assert not m1[2505:].any() and not v1[2505:].any() and p1[2507] == 0.0
        want_std = np.exp(p1[2503:2505].astype(np.float64)).astype(F)
        assert (np.abs(p1[2505:2507] - want_std) <= np.spacing(want_std)).all(), (p1[2503:2507], want_std)
        assert not np.array_equal(p1[2503:2505], p0[2503:2505])
    assert clipped >= 1
    # weights() is the same blob by key
    got = learner.weights()
    assert all(np.array_equal(bits(got[k]), bits(R.car_policy_unpack(p1)[k])) for k in Q.KEYS)
    learner.close()


def test_push_hands_the_master_blob_to_a_served_policy():
    _need_gpu()
    import competitive_rl_amd as crl
    from tests.test_hip_car_policy import reference, same_bits

    n, seed, base = 5, 6, 200
    env = crl.HipCarVecEnv(n, seed=4, env_id_base=base)
    policy = crl.CarPolicy(env, seed=seed)
    _, storage = filled()
    _, w, batches = Q.chosen()
    policy.add_network("learner", Q.base_weights())
    policy.assign(0, "learner"), policy.assign(1, "learner")
    env.reset()
    learner = crl.CarPPO(w, **Q.HYPER)
    learner.grad(storage, torch.from_numpy(batches[130].idx.astype(np.int64)).cuda())
    learner.step()
    learner.push(policy, "learner")
    mine, served = learner.weights(), policy.network_weights("learner")
    assert all(np.array_equal(bits(mine[k]), bits(served[k])) for k in Q.KEYS) and not policy.is_deterministic("learner")
    assert not np.array_equal(mine["log_std"], w["log_std"])
    acts = torch.zeros((n, 2, 2), device="cuda")
    obs, noise = torch.zeros((n, 2, 21), device="cuda"), torch.zeros((n, 2, 2), device="cuda")
    values, logp = policy.act_rollout(acts, obs_out=obs, noise_out=noise)
    state = env.get_state()
    tracks = Tracks(env)
    tracks.refresh(state)
    want = reference(state, tracks, {0: (mine, False)}, np.zeros((n, 2), np.int32), seed, base + np.arange(n), 0, z=noise.cpu().numpy())
    same_bits(acts.cpu().numpy(), want["u"], "actions")
    same_bits(values.cpu().numpy(), want["value"], "values")
    same_bits(logp.cpu().numpy(), want["log_prob"], "log-probs")
    learner.close(), policy.close(), env.close()


def test_state_dict_round_trips_and_refused_loads_leave_the_learner_alone():
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, batches = Q.chosen()
    idx = torch.from_numpy(batches[65].idx.astype(np.int64)).cuda()
    a = crl.CarPPO(w, **Q.HYPER)
    for _ in range(2):
        a.grad(storage, idx), a.step()
    sd = a.state_dict()
    assert sd["kind"] == "CarPPO" and sd["steps"] == 2 and set(sd["m"]) == set(Q.KEYS)
    b = crl.CarPPO(Q.base_weights())
    for bad in (dict(sd, kind="LightPPO"), dict(sd, steps=-1), dict(sd, m={k: v for k, v in sd["m"].items() if k != "fc1_b"}),
                dict(sd, weights=dict(sd["weights"], fc1_w=sd["weights"]["fc1_w"][:, :20])), dict(sd, hyper=dict(sd["hyper"], momentum=0.9))):
        with pytest.raises(ValueError, match="load_state_dict"):
            b.load_state_dict(bad)
    assert all(np.array_equal(bits(b.weights()[k]), bits(Q.base_weights()[k])) for k in Q.KEYS) and b.state_dict()["steps"] == 0
    b.load_state_dict(sd)
    with pytest.raises(crl._native.CrlError, match="no gradient"):
        b.step()
    for x in (a, b):
        x.grad(storage, idx), x.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["steps"] == sb["steps"] == 3 and sa["hyper"] == sb["hyper"]
    for part in ("weights", "m", "v"):
        assert all(np.array_equal(bits(sa[part][k]), bits(sb[part][k])) for k in Q.KEYS), part
    a.close(), b.close()

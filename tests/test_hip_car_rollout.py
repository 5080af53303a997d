"""The CarRacing learner's rollout storage on the device (include/crl.h "car rollout storage"; csrc/car_rollout.hip) against what
``CarPolicy.act_rollout`` and ``step_device`` produced and against the written rules -- bit for bit unless a bound is stated: the
gathered samples, ``live`` (assigned to the recorded network, not done, a track), the rows' dones (``done[e]`` or ``done_car[e][c]``),
returns and advantages against rules.gae_reference, normalised advantages against the float32 rule fed the device's own statistics;
the statistics over the LIVE samples against math.fsum values within the bounds of tests/test_hip_rollout_storage.py (the mean within
count * 2^-53 * sum|x| / L, the deviation at relative count * 2^-50).  Set-up as tests/test_hip_car_policy.py's open-loop test:
done_policy="car0" with car 1 of env 0 frozen off the playfield, every third env resetting inside the rollout, a per-env assignment
with -1 and a second network."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import car_policy_cases as CP  # noqa: E402
from tests.test_hip_car_drivers import Tracks, _need_gpu, bits  # noqa: E402

F = np.float32
PRE = 2  # steps in front of the rollout: car 1 of env 0 is done and frozen when step 0 is recorded


class Rolled:
    """An env, a policy with two sampling networks and a storage; ``roll()`` runs one rollout and keeps what every call produced"""

    def __init__(self, n, T, players, cars, normalize=True):
        import competitive_rl_amd as crl

        self.n, self.T, self.players, self.cars = n, T, players, cars
        self.env = crl.HipCarVecEnv(n, seed=11, env_id_base=1000, players=players, done_policy="car0" if players == 2 else "any")
        self.policy = crl.CarPolicy(self.env, seed=5)
        self.policy.add_network("learner", CP.random_weights(1, 2.0)), self.policy.add_network("other", CP.random_weights(2, 2.0))
        idx = np.arange(n)
        self.assign = np.stack([np.array([0, 1, 0, -1])[idx % 4], np.array([0, 0, -1, 1, 0])[idx % 5]], axis=1)[:, :players].astype(np.int32)
        for c in range(players):
            self.policy.assign(c, torch.as_tensor(self.assign[:, c].copy()).cuda())
        self.env.reset()
        st = self.env.get_state()
        if players == 2:
            for body in ("hull", "wheel"):
                st["car"][:, 1][body]["cx"][0] += 900.0  # env 0: car 1 leaves the playfield, done and frozen (done_policy="car0")
        self.soon = idx % 3 == 2  # (not env 0: its car 1 stays frozen for the whole rollout)
        st["elapsed"][self.soon] = 1000 - PRE - max(1, T // 2)  # these envs hit the TimeLimit inside the rollout
        self.env.set_state(st)
        self.tracks = Tracks(self.env)
        self.acts = torch.empty((n, players, 2), dtype=torch.float32, device="cuda")
        self.obs = torch.empty((n, players, 21), dtype=torch.float32, device="cuda")
        for _ in range(PRE):
            self.acts.fill_(0.1)
            self.env.step_device(self.acts, render=False)
        self.storage = crl.CarRolloutStorage(self.env, T, cars=cars, normalize_advantage=normalize)
        self.rows = n * len(cars)

    def act(self):
        self.acts.fill_(0.1)  # (what a car nobody serves drives with)
        return self.policy.act_rollout(self.acts, obs_out=self.obs)

    def roll(self):
        n, T, cars = self.n, self.T, list(self.cars)
        k = {name: [] for name in ("obs", "u", "value", "logp", "live", "rew", "done")}
        self.storage.begin()
        values, logp = self.act()
        for t in range(T):
            state = self.env.get_state()
            self.tracks.refresh(state)
            done_flag = np.stack([state["car"][:, c]["done"] for c in range(self.players)], axis=1)
            k["live"].append(((self.assign == 0) & (done_flag == 0) & (self.tracks.n > 0)[:, None])[:, cars])
            for name, x in (("obs", self.obs), ("u", self.acts), ("value", values), ("logp", logp)):
                k[name].append(x.cpu().numpy()[:, cars].copy())
            self.storage.record(t, self.policy, "learner", self.obs, self.acts, values, logp)
            _, rew, done = self.env.step_device(self.acts, render=False)
            done_car = self.env._info_snapshot()[0].cpu().numpy()
            k["rew"].append(rew.cpu().numpy()[:, cars].copy())
            k["done"].append((done.cpu().numpy()[:, None] != 0) | (done_car[:, cars] != 0))
            self.storage.outcome(t, rew, done)
            values, logp = self.act()
        self.last = values.cpu().numpy()[:, cars].copy()
        self.storage.finish(values)
        self.kept = {name: np.stack(v).reshape((T * self.rows,) + v[0].shape[2:]) for name, v in k.items()}
        self.env_done = int(sum(d.any(1).sum() for d in k["done"]))
        return self.kept

    def close(self):
        self.storage.close(), self.policy.close(), self.env.close()


def everything(r, seed=0):
    idx = np.random.RandomState(seed).permutation(r.T * r.rows).astype(np.int64)
    return idx, r.storage.gather(torch.from_numpy(idx).cuda())


@pytest.mark.parametrize("players,cars", [(1, (0,)), (2, (0,)), (2, (1,)), (2, (0, 1))])
@pytest.mark.parametrize("T", [1, 6])
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_gathered_samples_live_gae_and_statistics(n, T, players, cars):
    _need_gpu()
    from competitive_rl_amd import rules as R

    r = Rolled(n, T, players, cars)
    k = r.roll()
    total = T * r.rows
    idx, got = everything(r)
    for name, t in (("obs", got.obs), ("u", got.actions), ("value", got.values), ("logp", got.old_log_probs)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(k[name][idx])), name
    live = k["live"].astype(bool)
    assert np.array_equal(got.live.cpu().numpy().astype(bool), live[idx])
    # a dead sample is what act_rollout wrote for it: zeros where the car is done, log-prob 0 where nobody or the other network serves
    assert n == 1 or 0 < live.sum() < total
    adv, ret = R.gae_reference(k["rew"].reshape(T, r.rows), k["value"].reshape(T, r.rows), k["done"].reshape(T, r.rows), r.last.reshape(-1), 0.99, 0.95)
    adv, ret = adv.reshape(-1), ret.reshape(-1)
    assert np.array_equal(bits(got.returns.cpu().numpy()), bits(ret[idx]))
    # the statistics over the live samples
    x = [float(v) for v in adv[live]]
    L = len(x)
    mean = math.fsum(x) / L if L else 0.0  # (the rule: 0 where nothing is live, and no deviation below two samples)
    std = math.sqrt(math.fsum((v - mean) ** 2 for v in x) / (L - 1)) if L > 1 else 0.0
    got_mean, got_std, got_live = r.storage.stats()
    sum_abs = math.fsum(abs(v) for v in x)
    print("car rollout statistics n %d T %d cars %s: L %d of %d, mean error %.3g (bound %.3g)  std relative error %.3g (bound %.3g)" % (
        n, T, cars, L, total, abs(got_mean - mean), total * 2.0 ** -53 * sum_abs / max(L, 1), abs(got_std - std) / std if std else 0.0, total * 2.0 ** -50))
    assert got_live == L
    assert abs(got_mean - mean) <= total * 2.0 ** -53 * sum_abs / max(L, 1)
    assert abs(got_std - std) <= total * 2.0 ** -50 * std
    want = ((adv - F(got_mean)) / (F(got_std) + F(1e-5))).astype(F)
    assert np.array_equal(bits(got.advantages.cpu().numpy()), bits(want[idx]))
    # a second run gives the same bits
    r.storage.finish(torch.from_numpy(np.ascontiguousarray(_full(r, r.last))).cuda())
    assert r.storage.stats() == (got_mean, got_std, got_live)
    assert np.array_equal(bits(r.storage.gather(torch.from_numpy(idx).cuda(), fields=("advantages",)).advantages.cpu().numpy()), bits(want[idx]))
    # what the set-up is there for
    if players == 2 and 1 in cars:
        frozen = k["done"].reshape(T, n, len(cars))[:, 0, list(cars).index(1)]
        assert frozen.all() and not k["live"].reshape(T, n, len(cars))[:, 0, list(cars).index(1)].any()  # done_car keeps a frozen car's rows done
    assert r.env_done >= int(r.soon.sum())
    r.close()


def _full(r, rows_values):
    """(N, C) values of the stored cars back in an (N, P) tensor"""
    out = np.zeros((r.n, r.players), F)
    out[:, list(r.cars)] = rows_values.reshape(r.n, len(r.cars))
    return out


def test_the_state_machine_refuses_out_of_order_calls_and_a_deterministic_slot():
    _need_gpu()
    from competitive_rl_amd._native import CrlError

    r = Rolled(3, 2, 2, (0, 1))
    st, idx = r.storage, torch.zeros(1, dtype=torch.int64, device="cuda")
    values, logp = r.act()
    rew, done = torch.zeros((3, 2), device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda")
    with pytest.raises(CrlError, match="crl_car_rollout_finish"):
        st.finish()
    with pytest.raises(CrlError, match="crl_car_rollout_gather"):
        st.gather(idx)
    with pytest.raises(CrlError, match="crl_car_rollout_outcome"):
        st.outcome(0, rew, done)
    st.begin()
    with pytest.raises(CrlError, match="not the next step"):
        st.record(1, r.policy, "learner", r.obs, r.acts, values, logp)
    st.record(0, r.policy, "learner", r.obs, r.acts, values, logp)
    with pytest.raises(CrlError, match="not the next step"):
        st.record(0, r.policy, "learner", r.obs, r.acts, values, logp)
    with pytest.raises(CrlError, match="crl_car_rollout_outcome"):
        st.outcome(1, rew, done)
    st.outcome(0, rew, done)
    with pytest.raises(CrlError, match="crl_car_rollout_outcome"):
        st.outcome(0, rew, done)
    with pytest.raises(CrlError, match="1 of 2 steps"):
        st.finish()
    r.policy.add_network("mean", CP.random_weights(3), deterministic=True)
    with pytest.raises(CrlError, match="deterministic"):
        st.record(1, r.policy, "mean", r.obs, r.acts, values, logp)
    st.record(1, r.policy, "learner", r.obs, r.acts, values, logp)
    with pytest.raises(CrlError, match="not the next step"):
        st.record(2, r.policy, "learner", r.obs, r.acts, values, logp)
    st.outcome(1, rew, done)
    st.finish()
    with pytest.raises(CrlError, match="finished"):
        st.record(0, r.policy, "learner", r.obs, r.acts, values, logp)
    assert st.gather(idx).obs.shape == (1, 21)
    st.begin()  # rewinds
    st.record(0, r.policy, "learner", r.obs, r.acts, values, logp)
    with pytest.raises(AssertionError):
        st.record(1, r.policy, "learner", r.obs[:, :1], r.acts, values, logp)
    r.close()


def test_a_mask_naming_a_missing_car_is_refused():
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd._native import CrlError

    env = crl.HipCarVecEnv(2, seed=1, players=1)
    with pytest.raises(CrlError, match="cars_mask"):
        crl.CarRolloutStorage(env, 3, cars=(0, 1))
    with pytest.raises(ValueError):
        crl.CarRolloutStorage(env, 3, cars=(2,))
    st = crl.CarRolloutStorage(env, 3, cars=(0,))
    assert st.rows == 2 and st.nbytes() == 3 * 2 * 128 + 2 * 4 + (3 + 512) * 8
    st.close(), env.close()


@pytest.mark.parametrize("contents", [True, False])
def test_state_dict_round_trips_into_a_fresh_object(contents):
    _need_gpu()
    import competitive_rl_amd as crl

    r = Rolled(3, 6, 2, (0, 1))
    r.roll()
    idx, want = everything(r)
    sd = r.storage.state_dict(contents=contents)
    fresh = crl.CarRolloutStorage(r.env, 6, cars=(0, 1), gamma=0.5, normalize_advantage=False)
    fresh.load_state_dict(sd)
    assert (fresh.gamma, fresh.normalize_advantage) == (0.99, True)
    if contents:
        assert sd["contents"]["lines"].shape == (6 * 6, 32) and sd["state"] == "finished"
        got = fresh.gather(torch.from_numpy(idx).cuda())
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert fresh.stats() == r.storage.stats()
    else:
        assert sd["contents"] is None
        with pytest.raises(crl._native.CrlError, match="crl_car_rollout_gather"):
            fresh.gather(torch.from_numpy(idx).cuda())
        fresh.begin()
    # the middle of a rollout: only with contents, and the remaining steps give the uninterrupted run's bits
    r.storage.begin()
    values, logp = r.act()
    r.storage.record(0, r.policy, "learner", r.obs, r.acts, values, logp)
    with pytest.raises(ValueError, match="middle of a rollout"):
        r.storage.state_dict(contents=False)
    mid = r.storage.state_dict()
    assert mid["state"] == "active" and mid["step"] == 1 and mid["outcomes"] == 0 and mid["contents"]["lines"].shape == (6, 32)
    fresh.load_state_dict(mid)
    for bad in (dict(mid, num_envs=4), dict(mid, cars=(0,)), dict(mid, step=7), dict(mid, contents=dict(mid["contents"], lines=mid["contents"]["lines"][:3])),
                dict(mid, kind="RolloutStorage"), dict(mid, contents=None)):
        with pytest.raises(ValueError, match="load_state_dict"):
            fresh.load_state_dict(bad)
    for st in (r.storage, fresh):  # (the refused loads left `fresh` as it was: step 0 recorded)
        rew = torch.full((3, 2), 0.5, device="cuda")
        for t in range(6):
            if t:
                st.record(t, r.policy, "learner", r.obs, r.acts, values, logp)
            st.outcome(t, rew, torch.zeros(3, dtype=torch.uint8, device="cuda"))
        st.finish(values)
    a, b = r.storage.gather(torch.from_numpy(idx).cuda()), fresh.gather(torch.from_numpy(idx).cuda())
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    fresh.close(), r.close()


def made_up_lines(rows, T, seed):
    """Host data of an unfinished rollout in the shape of tests/car_ppo_cases.Pool.lines(): uint32 [T * rows, 32] with made-up
    observations, actions, log-probs, values and rewards, 20 % dones and every seventh sample dead (zeros, as the device stores a done
    car); returns and advantages are left at 0 for ``finish``.  Also (live [T * rows], rewards, values, dones [T, rows], last [rows])."""
    rs = np.random.RandomState(seed)
    S = T * rows
    live = np.arange(S) % 7 != 6
    ln = np.zeros((S, 32), F)
    ln[:, :26] = rs.standard_normal((S, 26)).astype(F)
    ln[~live, :25] = 0
    dones = rs.random_sample((T, rows)) < 0.2
    last = rs.standard_normal(rows).astype(F)
    out = ln.view(np.uint32)
    out[:, 28] = live.astype(np.uint32) | (dones.reshape(-1).astype(np.uint32) << 1)
    return out, live, ln[:, 25].reshape(T, rows).copy(), ln[:, 24].reshape(T, rows).copy(), dones, last


def test_statistics_where_a_lane_takes_a_second_trip():
    """260 rows x 253 steps = 65 780 samples, just over the 65 536 that 256 workgroups of 256 lanes cover in one trip: the first 244
    lanes of workgroup 0 add a second sample.  Loaded as an active rollout whose steps all have their outcome; no env step."""
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd import rules as R

    n, T = 130, 253
    rows, total = 2 * n, 2 * n * T
    assert 65536 < total < 65536 + 256
    lines, live, rew, val, dones, last = made_up_lines(rows, T, 31)
    env = crl.HipCarVecEnv(n, seed=2)
    st = crl.CarRolloutStorage(env, T, cars=(0, 1))
    st.load_state_dict({"kind": "CarRolloutStorage", "num_steps": T, "num_envs": n, "players": 2, "cars": (0, 1), "gamma": 0.99, "gae_lambda": 0.95,
                        "normalize_advantage": True, "state": "active", "step": T, "outcomes": T,
                        "contents": {"lines": lines, "stats": np.zeros(3), "normalized": False}})
    st.finish(torch.from_numpy(last.reshape(n, 2)).cuda())
    adv, ret = R.gae_reference(rew, val, dones, last, 0.99, 0.95)
    adv, ret = adv.reshape(-1), ret.reshape(-1)
    stored = st.state_dict()["contents"]["lines"]
    assert np.array_equal(stored[:, 26], bits(ret)) and np.array_equal(stored[:, 27], bits(adv))
    assert np.array_equal(np.delete(stored, (26, 27), axis=1), np.delete(lines, (26, 27), axis=1))
    x = [float(v) for v in adv[live]]
    L = len(x)
    mean = math.fsum(x) / L
    std = math.sqrt(math.fsum((v - mean) ** 2 for v in x) / (L - 1))
    got_mean, got_std, got_live = st.stats()
    sum_abs = math.fsum(abs(v) for v in x)
    print("car rollout statistics, second trip: L %d of %d, mean error %.3g (bound %.3g)  std relative error %.3g (bound %.3g)" % (
        L, total, abs(got_mean - mean), total * 2.0 ** -53 * sum_abs / L, abs(got_std - std) / std, total * 2.0 ** -50))
    assert got_live == L == total - total // 7
    assert abs(got_mean - mean) <= total * 2.0 ** -53 * sum_abs / L
    assert abs(got_std - std) <= total * 2.0 ** -50 * std
    idx = np.random.RandomState(0).permutation(total).astype(np.int64)
    got = st.gather(torch.from_numpy(idx).cuda(), fields=("returns", "advantages", "live"))
    want = ((adv - F(got_mean)) / (F(got_std) + F(1e-5))).astype(F)
    assert np.array_equal(bits(got.returns.cpu().numpy()), bits(ret[idx]))
    assert np.array_equal(bits(got.advantages.cpu().numpy()), bits(want[idx]))
    assert np.array_equal(got.live.cpu().numpy().astype(bool), live[idx])
    st.close(), env.close()

"""The car policy on the device (include/crl.h "car policy"; csrc/car_policy.hip) against the numpy restatements
``rules.car_obs_reference`` / ``car_mlp_reference`` / ``car_policy_reference`` -- tolerance 0 but for the noise z, which lies within the
header's derived bound of a float64 Box-Muller: open loop on the device's own state through auto-resets, frozen cars and cars off the
track; sampling; a weight reload between two calls; shards; closed loop against the CPU checker; ``CarDrivers`` beside it; resume; a
held side stream; ``make_competitive_car_racing(weights)``."""
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import car_policy_cases as CP  # noqa: E402
from tests.test_hip_car_drivers import SENTINEL, Tracks, _need_gpu, bits  # noqa: E402

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "car_policy_clone.npz")


def clone_weights():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def reference(state, tracks, nets, assign, seed, gid, call, players=2, z=None):
    """What ``act_rollout`` must leave behind a SENTINEL-filled action tensor: nets = {slot: (weights, deterministic)}, assign int
    [N, players]; z: the device's noise [N, players, 2] (None: rules.car_policy_noise).  Returns dict of arrays."""
    from competitive_rl_amd import rules as R

    n = len(state)
    out = dict(u=np.full((n, players, 2), SENTINEL, F), value=np.zeros((n, players), F), log_prob=np.zeros((n, players), F),
               z=np.zeros((n, players, 2), F), obs=np.zeros((n, players, 21), F))
    for c in range(players):
        out["obs"][:, c] = CP.obs_of_state(state, c, tracks.boxes, tracks.n, players)
        live = (state["car"][:, c]["done"] == 0) & (tracks.n > 0)
        for slot, (w, det) in nets.items():
            rows = assign[:, c] == slot
            if rows.any():
                r = R.car_policy_reference(w, out["obs"][:, c], live, det, seed, gid, c, call, None if z is None else z[:, c])
                for k in ("u", "value", "log_prob", "z"):
                    out[k][rows, c] = r[k][rows]
    return out


def same_bits(got, want, what):
    bad = np.nonzero((bits(got) != bits(want)).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, (what, "envs", bad[:8], np.asarray(got)[bad[:2]], np.asarray(want)[bad[:2]])


@pytest.mark.parametrize("n,players", [(1, 2), (3, 2), (3, 1), (65, 2), (130, 2)])
def test_open_loop_equals_the_rule_bit_for_bit(n, players):
    _need_gpu()
    import competitive_rl_amd as crl

    base, seed, steps = 1000, 5, 40
    env = crl.HipCarVecEnv(n, seed=11, env_id_base=base, players=players, done_policy="car0" if players == 2 else "any")
    policy = crl.CarPolicy(env, seed=seed)
    nets = {0: (CP.random_weights(1, 2.0), True), 1: (clone_weights(), True)}
    assert policy.add_network("random", nets[0][0], deterministic=True) == 0 and policy.add_network("clone", nets[1][0], deterministic=True) == 1
    assert policy.network_names() == ("random", "clone") and policy.is_deterministic("clone")
    idx = np.arange(n)
    assign = np.stack([np.array([1, 0, -1])[idx % 3], np.array([0, -1, 1, 1, 0])[idx % 5]], axis=1)[:, :players].astype(np.int32)
    for c in range(players):
        policy.assign(c, torch.as_tensor(assign[:, c].copy()).cuda())
    assert np.array_equal(policy.assignment().cpu().numpy(), assign)
    env.reset()
    st = env.get_state()
    far = 0  # env 0: car 1 leaves the playfield and stays in the world, done and frozen (done_policy="car0")
    off = (1 % n) if n > 1 else None  # another env: car 0 far off its track, inside the playfield
    for body in ("hull", "wheel"):
        if players == 2:
            st["car"][:, 1][body]["cx"][far] += 900.0
        if off is not None:
            st["car"][:, 0][body]["cx"][off] += 40.0
            st["car"][:, 0][body]["cy"][off] -= 35.0
    soon = idx % 3 == 0  # these envs hit the TimeLimit at step 12: the auto-reset lays a new track
    st["elapsed"][soon] = 1000 - 12
    env.set_state(st)
    tracks = Tracks(env)
    gid = base + idx
    acts = torch.empty((n, players, 2), dtype=torch.float32, device="cuda")
    obs = torch.empty((n, players, 21), dtype=torch.float32, device="cuda")
    noise = torch.empty((n, players, 2), dtype=torch.float32, device="cuda")
    resets = frozen = 0
    for t in range(steps + 1):
        acts.fill_(SENTINEL), obs.fill_(SENTINEL), noise.fill_(SENTINEL)
        seen = policy.observe()
        values, logp = policy.act_rollout(acts, obs_out=obs, noise_out=noise)
        state = env.get_state()
        tracks.refresh(state)
        want = reference(state, tracks, nets, assign, seed, gid, t, players)
        same_bits(obs.cpu().numpy(), want["obs"], ("obs", t))
        assert torch.equal(seen.view(torch.int32), obs.view(torch.int32))
        got = acts.cpu().numpy()
        same_bits(got, want["u"], ("actions", t))  # (deterministic: the mean itself)
        same_bits(values.cpu().numpy(), want["value"], ("values", t))
        assert not logp.any() and not noise.any()
        assert (got[assign < 0] == SENTINEL).all() and (got[assign >= 0] != SENTINEL).all()
        if players == 2:
            frozen += int(state["car"][far, 1]["done"] == 1)
            if state["car"][far, 1]["done"] == 1:
                assert not obs[far, 1].any() and obs[far, 0, 20] == 0
                if assign[far, 1] >= 0:
                    assert got[far, 1].tolist() == [0.0, 0.0] and values[far, 1] == 0
        if t == steps:
            break
        a = torch.where(acts == SENTINEL, torch.full_like(acts, 0.1), acts)
        _, _, done = env.step_device(a, render=False)
        resets += int(done.sum())
    assert policy.calls == steps + 1  # (observe does not count)
    assert resets >= int(soon.sum()) and (tracks.episode[soon] >= 2).all()
    if players == 2:
        assert frozen >= 10
    policy.close(), env.close()


def _set_counters(policy, seed, calls):
    from competitive_rl_amd import _native as N

    N.check(policy._L.crl_car_policy_set_counters(policy._h, seed, calls))


def test_sampled_actions_noise_within_the_bound_and_the_rest_bit_for_bit():
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd import rules as R

    n, base, seed = 65, 1000, (7 << 32) | 9
    env = crl.HipCarVecEnv(n, seed=3, env_id_base=base, done_policy="car0")
    policy = crl.CarPolicy(env, seed=seed)
    nets = {0: (CP.random_weights(2, 2.0), False), 1: (CP.random_weights(3, 1.0, log_std=(0.5, -1.5)), False)}
    policy.add_network("a", nets[0][0]), policy.add_network("b", nets[1][0])
    assert not policy.is_deterministic("a")
    idx = np.arange(n)
    assign = np.stack([idx % 2, np.array([1, 0, -1])[idx % 3]], axis=1).astype(np.int32)
    for c in range(2):
        policy.assign(c, torch.as_tensor(assign[:, c].copy()).cuda())
    env.reset()
    st = env.get_state()
    for body in ("hull", "wheel"):
        st["car"][:, 1][body]["cx"][0] += 900.0  # a done car from the second step on
    env.set_state(st)
    tracks = Tracks(env)
    gid = base + idx
    acts = torch.empty((n, 2, 2), dtype=torch.float32, device="cuda")
    noise = torch.empty((n, 2, 2), dtype=torch.float32, device="cuda")
    worst, kept = 0.0, None
    for t in range(6):
        acts.fill_(SENTINEL)
        values, logp = policy.act_rollout(acts, noise_out=noise)
        state = env.get_state()
        tracks.refresh(state)
        z = noise.cpu().numpy()
        want = reference(state, tracks, nets, assign, seed, gid, t, z=z)
        for c in range(2):  # the device's z against the float64 value, within the header's bound
            Z, bound = R.car_policy_noise_bound(seed, gid, c, t)
            rows = (assign[:, c] >= 0) & (state["car"][:, c]["done"] == 0)
            assert rows.sum() > 20 and (np.abs(z[rows, c] - Z[rows]) <= bound[rows]).all(), (t, c)
            assert (z[~rows, c] == 0).all()
            worst = max(worst, float((np.abs(z[rows, c] - Z[rows]) / bound[rows]).max()))
        same_bits(acts.cpu().numpy(), want["u"], ("actions", t))  # given the device's own z: the written expressions
        same_bits(logp.cpu().numpy(), want["log_prob"], ("log_prob", t))
        same_bits(values.cpu().numpy(), want["value"], ("values", t))
        if t == 3:
            kept = (acts.clone(), values.clone(), logp.clone(), noise.clone())
            _set_counters(policy, seed, 3)  # the same call again
            acts.fill_(SENTINEL)
            v2, l2 = policy.act_rollout(acts, noise_out=noise)
            for a, b in zip(kept, (acts, v2, l2, noise)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert policy.calls == 4
        env.step_device(torch.where(acts == SENTINEL, torch.full_like(acts, 0.1), acts), render=False)
    print("device noise against float64 Box-Muller: largest error / bound %.3f" % worst)
    assert state["car"][0, 1]["done"] == 1 and float(logp.abs().max()) > 0
    # set_sampling: the mean from the next call on
    policy.set_sampling("a", deterministic=True)
    acts.fill_(SENTINEL)
    values, logp = policy.act_rollout(acts, noise_out=noise)
    state = env.get_state()
    tracks.refresh(state)
    want = reference(state, tracks, {0: (nets[0][0], True), 1: nets[1]}, assign, seed, gid, 6, z=noise.cpu().numpy())
    same_bits(acts.cpu().numpy(), want["u"], "after set_sampling")
    assert not logp[torch.as_tensor(assign == 0).cuda()].any()
    policy.close(), env.close()


def test_update_network_between_two_calls_without_a_synchronisation():
    _need_gpu()
    import competitive_rl_amd as crl

    n = 33
    env = crl.HipCarVecEnv(n, seed=4, env_id_base=1000)
    policy = crl.CarPolicy(env, seed=1)
    old, new = CP.random_weights(5, 2.0), CP.random_weights(6, 2.0)
    policy.add_network("learner", old, deterministic=True)
    policy.assign(0, "learner"), policy.assign(1, "learner")
    env.reset()
    tracks = Tracks(env)
    state = env.get_state()
    tracks.refresh(state)
    a1, a2 = torch.zeros((n, 2, 2), device="cuda"), torch.zeros((n, 2, 2), device="cuda")
    torch.cuda.synchronize()
    v1, _ = policy.act_rollout(a1)
    policy.update_network("learner", new)  # (nothing waits between the three calls)
    v2, _ = policy.act_rollout(a2)
    assign = np.zeros((n, 2), np.int32)
    for acts, values, w, call in ((a1, v1, old, 0), (a2, v2, new, 1)):
        want = reference(state, tracks, {0: (w, True)}, assign, 1, 1000 + np.arange(n), call)
        same_bits(acts.cpu().numpy(), want["u"], ("actions", call))
        same_bits(values.cpu().numpy(), want["value"], ("values", call))
    assert not torch.equal(a1, a2)
    held = policy.network_weights("learner")
    assert all(np.array_equal(bits(held[k]), bits(new[k])) for k in new) and policy.is_deterministic("learner")
    # the C entry points take host memory as well (include/crl.h: "host or device")
    import ctypes

    from competitive_rl_amd import _native as N
    from competitive_rl_amd import rules as R

    blob, back = R.car_policy_pack(old), np.zeros(N.CRL_CAR_POLICY_BLOB_FLOATS, F)
    N.check(policy._L.crl_car_policy_set_weights(policy._h, 0, blob.ctypes.data_as(ctypes.c_void_p), 1, policy._stream()))
    N.check(policy._L.crl_car_policy_get_weights(policy._h, 0, back.ctypes.data_as(ctypes.c_void_p), None, policy._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(back), bits(blob))
    held = policy.network_weights("learner")
    assert all(np.array_equal(bits(held[k]), bits(old[k])) for k in old)
    with pytest.raises(ValueError, match="Unknown car policy network"):
        policy.update_network("nobody", new)
    with pytest.raises(ValueError, match="exists"):
        policy.add_network("learner", new)
    with pytest.raises(AssertionError):
        policy.act(torch.zeros((n, 2, 3), device="cuda"))
    with pytest.raises(AssertionError):
        policy.act_rollout(a1, obs_out=torch.zeros((n, 2, 20), device="cuda"))
    policy.close(), env.close()


def test_shards_act_as_the_whole_batch():
    _need_gpu()
    import competitive_rl_amd as crl

    def make(n, base):
        env = crl.HipCarVecEnv(n, seed=21, env_id_base=base)
        p = crl.CarPolicy(env, seed=8)
        p.add_network("a", CP.random_weights(7, 2.0)), p.add_network("b", clone_weights())
        p.set_sampling("b", deterministic=False)
        p.assign(0, "a"), p.assign(1, "b")
        env.reset()
        return env, p, torch.zeros((n, 2, 2), device="cuda"), torch.zeros((n, 2, 2), device="cuda"), torch.zeros((n, 2, 21), device="cuda")

    whole, parts = make(130, 0), [make(65, 0), make(65, 65)]
    for t in range(10):
        outs = []
        for env, p, a, z, o in [whole] + parts:
            v, lp = p.act_rollout(a, obs_out=o, noise_out=z)
            outs.append((a, v, lp, z, o))
        for k in range(5):
            cut = torch.cat([outs[1][k], outs[2][k]])
            assert torch.equal(outs[0][k].view(torch.int32), cut.view(torch.int32)), (t, k)
        for env, p, a, z, o in [whole] + parts:
            env.step_device(a, render=False)
    assert len(torch.unique(whole[3][:, 0, 0])) > 100  # (one draw per env)
    for env, p, a, z, o in [whole] + parts:
        p.close(), env.close()


def test_closed_loop_equals_the_cpu_loop():
    """16 envs x 200 steps, car 0 under the stored clone and car 1 under a fixed random net, both deterministic, through step_device
    without a host read inside the loop, against oracle.car_oracle.CarBatch driven by rules.car_policy_reference on the same tracks.
    The env is bit-exact against the CPU checker (tests/test_hip_car_episodes.py), so a difference is the policy's."""
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd import rules as R
    from oracle import car_oracle as co
    from tests.car_scenarios import make_oracle_envs
    from tests.test_hip_car_episodes import batch_to_hip_state

    n, steps = 16, 200
    seeds = make_oracle_envs(n, seed0=2)
    B = co.CarBatch(n)
    for i in range(n):
        B.E[i] = seeds[i].e
    env = crl.HipCarVecEnv(n, seed=1)
    env.reset()
    for j in range(n):
        e = seeds[j].e
        nt = int(e["trk"]["n"])
        border = np.where(e["trk"]["border"][:nt] > 0, np.where(np.arange(nt) % 2 == 0, 1, 2), 0).astype(np.uint8)
        env.set_track(j, e["trk"]["tile"][:nt], e["trk"]["border_poly"][:nt], border, e["trk"]["track"][0][1:4].astype(np.float32))
    env.set_state(batch_to_hip_state(B.E))
    nets = [clone_weights(), CP.random_weights(11, 1.0)]
    policy = crl.CarPolicy(env, seed=13)
    policy.add_network("clone", nets[0], deterministic=True), policy.add_network("random", nets[1], deterministic=True)
    policy.assign(0, "clone"), policy.assign(1, "random")
    acts = torch.zeros((n, 2, 2), device="cuda")
    rec_a = torch.zeros((steps, n, 2, 2), device="cuda")
    rec_r = torch.zeros((steps, n, 2), device="cuda")
    any_done = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    for t in range(steps):  # (device only)
        policy.act(acts)
        rec_a[t].copy_(acts)
        _, rew, done = env.step_device(acts, render=False)
        rec_r[t].copy_(rew)
        any_done |= done
    got_a, got_r = rec_a.cpu().numpy(), rec_r.cpu().numpy()
    assert not bool(any_done.any()), "an episode ended: the device laid a new track, the CPU loop did not"
    nt = B.E["trk"]["n"].astype(np.int64)
    boxes = B.E["tile_aabb"].copy()
    for t in range(steps):
        a = np.zeros((n, 2, 2), F)
        for c in range(2):
            a[:, c] = R.car_policy_reference(nets[c], CP.obs_of_batch(B.E, c, boxes, nt), B.E["done"][:, c] == 0, True)["u"]
        same_bits(got_a[t], a, ("actions", t))
        r, _ = B.step(a.astype(np.float64))
        assert np.array_equal(bits(got_r[t]), bits(r.astype(F))), ("rewards", t)
    st = env.get_state()
    assert np.array_equal(st["car"]["tile_visited_count"], B.E["tile_visited_count"])
    assert (B.E["tile_visited_count"][:, 0] > 10).all()  # (the clone drove: 4 s from a standing start)
    policy.close(), env.close()


def test_car_drivers_and_car_policy_share_one_action_tensor():
    _need_gpu()
    import competitive_rl_amd as crl

    n = 37
    env = crl.HipCarVecEnv(n, seed=6)
    drivers, policy = crl.CarDrivers(env, seed=2), crl.CarPolicy(env, seed=2)
    policy.add_network("net", CP.random_weights(8, 2.0))
    idx = torch.arange(n, device="cuda")
    # car 0: the net in even envs, RULE_BASED in envs 1 mod 4, nobody in envs 3 mod 4;  car 1: RANDOM in envs 0 mod 3, else the net
    none = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    policy.assign(0, torch.where(idx % 2 == 0, torch.zeros_like(none), none))
    drivers.assign(0, torch.where(idx % 4 == 1, torch.ones_like(none), none))
    drivers.assign(1, torch.where(idx % 3 == 0, torch.zeros_like(none), none))
    policy.assign(1, torch.where(idx % 3 == 0, none, torch.zeros_like(none)))
    env.reset()
    for t in range(5):
        alone_d, alone_p, both = (torch.full((n, 2, 2), SENTINEL, device="cuda") for _ in range(3))
        drivers.act(alone_d)
        policy.act(alone_p)
        _set_counters(policy, 2, t)
        from competitive_rl_amd import _native as N

        N.check(drivers._L.crl_car_driver_set_counters(drivers._h, 2, t))
        drivers.act(both), policy.act(both)
        by_d, by_p = alone_d != SENTINEL, alone_p != SENTINEL
        assert not bool((by_d & by_p).any()) and int(by_d.sum()) > n // 2 and int(by_p.sum()) > n
        want = torch.where(by_d, alone_d, torch.where(by_p, alone_p, torch.full_like(both, SENTINEL)))
        assert torch.equal(both.view(torch.int32), want.view(torch.int32)), t
        assert bool((both[3::4, 0] == SENTINEL).all())
        env.step_device(torch.where(both == SENTINEL, torch.full_like(both, 0.1), both), render=False)
    drivers.close(), policy.close(), env.close()


def test_resume_from_state_dicts_gives_the_uninterrupted_bytes():
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps, cut = 6, 30, 10
    nets = dict(a=CP.random_weights(12, 2.0), b=clone_weights())

    def make(policy_seed):
        env = crl.HipCarVecEnv(n, seed=9)
        env.reset()
        return env, crl.CarPolicy(env, seed=policy_seed), torch.zeros((n, 2, 2), device="cuda")

    def run(p, acts):
        v, lp = p.act_rollout(acts)
        return torch.cat([acts.reshape(n, -1), v, lp], dim=1).clone()

    env, p, acts = make(17)
    p.add_network("a", nets["a"]), p.add_network("b", nets["b"], deterministic=True)
    p.assign(0, "a")
    p.assign(1, torch.as_tensor(np.array([1, 0, 1, 0, -1, 0], np.int32)).cuda())
    want, saved = [], None
    for t in range(steps):
        if t == cut:
            saved = (env.state_dict(), p.state_dict())
        want.append(run(p, acts))
        _, _, done = env.step_device(acts, render=False)
        assert not bool(done.any())
    p.close(), env.close()
    sd = saved[1]
    assert sd["calls"] == cut and sd["seed"] == 17 and set(sd["networks"]) == {"a", "b"} and sd["networks"]["b"]["deterministic"] is True
    assert all(np.array_equal(bits(sd["networks"]["a"]["weights"][k]), bits(nets["a"][k])) for k in nets["a"])
    env, p, acts = make(0)  # (the same tracks: episode 1 of the same seed)
    p.add_network("other", CP.random_weights(13))
    before = p.state_dict()
    bad_net = dict(sd["networks"]["a"], weights=dict(sd["networks"]["a"]["weights"], fc1_b=np.zeros(99, F)))
    broken = [dict(sd, num_envs=n + 1), dict(sd, calls=-1), dict(sd, assignment=sd["assignment"][:3]), dict(sd, kind="CarDrivers"),
              dict(sd, networks=dict(sd["networks"], a=bad_net)), dict(sd, networks=dict(a=dict(sd["networks"]["a"], slot=3))),
              dict(sd, networks=dict(sd["networks"], a=dict(sd["networks"]["a"], deterministic=2)))]
    for bad in broken:
        with pytest.raises(ValueError, match="load_state_dict"):
            p.load_state_dict(bad)
        after = p.state_dict()
        assert set(after["networks"]) == {"other"} and after["calls"] == 0 and after["seed"] == 0
        assert np.array_equal(after["assignment"], before["assignment"])
        assert np.array_equal(after["networks"]["other"]["weights"]["fc1_w"], before["networks"]["other"]["weights"]["fc1_w"])
    env.load_state_dict(saved[0])
    p.load_state_dict(sd)
    assert p.network_names() == ("a", "b") and p.is_deterministic("b") and not p.is_deterministic("a")
    for t in range(cut, steps):
        got = run(p, acts)
        assert torch.equal(got.view(torch.int32), want[t].view(torch.int32)), t
        env.step_device(acts, render=False)
    p.close(), env.close()


# ---- side stream: the helper pattern of tests/stream_cases.py (a reference run on the default stream, a held run on a side stream)
POLICY_STEPS = 10


class CarPolicyCase:
    """CarPolicy beside a HipCarVecEnv.  Calls of a pass: POLICY_STEPS x (act_rollout, step_device), an ``observe`` every step, an
    ``update_network`` after step 2, a ``set_sampling`` and an ``assign`` by name after step 4 and an ``assign`` by device tensor after
    step 6.  ``reset()`` and ``add_network`` stay in front of the chain."""
    name = "car-policy"

    def build(self):
        import competitive_rl_amd as crl

        o = types.SimpleNamespace()
        o.n = 9
        o.env = crl.HipCarVecEnv(o.n, seed=31, done_policy="car0")
        o.policy = crl.CarPolicy(o.env, seed=2)
        o.policy.add_network("a", CP.random_weights(14, 2.0)), o.policy.add_network("b", clone_weights(), deterministic=True)
        o.policy.assign(0, "a"), o.policy.assign(1, "b")
        o.env.reset()
        st = o.env.get_state()
        st["elapsed"][::2] = 1000 - 7  # auto-resets inside both passes
        st["elapsed"][1::2] = 1000 - POLICY_STEPS - 4
        o.env.set_state(st)
        o.acts = torch.zeros((o.n, 2, 2), device="cuda")
        o.obs = torch.zeros((o.n, 2, 21), device="cuda")
        o.ids = torch.as_tensor(np.array([0, 1, 1, -1, 0, 1, 0, 0, 1], np.int32)).cuda()
        o.new = [CP.random_weights(15 + k, 2.0) for k in range(2)]
        return o

    def chain(self, rec, o, k):
        with rec.on("A"):
            for t in range(POLICY_STEPS):
                seen = rec.call("observe", o.policy.observe, o.obs)
                rec.keep("step%d.obs_seen" % t, seen)
                values, logp = rec.call("act_rollout", o.policy.act_rollout, o.acts)
                for name, x in (("actions", o.acts), ("values", values), ("logp", logp)):
                    rec.keep("step%d.%s" % (t, name), x)
                buf, rew, done = rec.call("step_device", o.env.step_device, o.acts)
                for name, x in (("obs", buf), ("rew", rew), ("done", done)):
                    rec.keep("step%d.%s" % (t, name), x)
                if t == 2:
                    rec.call("update_network", o.policy.update_network, "a", o.new[k])
                elif t == 4:
                    rec.call("set_sampling", o.policy.set_sampling, "b", k == 0)
                    rec.call("assign(name)", o.policy.assign, 1, "a" if k else "b")
                elif t == 6:
                    rec.call("assign(tensor)", o.policy.assign, 0, o.ids)

    def finish(self, rec, o):
        rec.out["env_state"] = o.env.get_state()
        rec.out["assignment"] = o.policy.assignment().cpu().numpy()
        rec.out["weights"] = o.policy.network_weights("a")["fc1_w"]

    def close(self, o):
        o.policy.close(), o.env.close()


def test_act_and_step_on_a_held_side_stream_equal_the_default_stream():
    _need_gpu()
    from tests import stream_cases as SC

    case = CarPolicyCase()
    ref = SC.reference_run(case)
    side = SC.held_run(case, {"A": SC.pick_streams(1)[0]})
    assert SC.same(ref.out, side.out) == []
    dones = [ref.out["%d:step%d.done" % (k, t)] for k in range(2) for t in range(POLICY_STEPS)]
    assert sum(int(d.sum()) for d in dones) >= 9  # (episodes ended inside the chain)
    assert not torch.equal(ref.out["1:step2.actions"][:, 0], ref.out["1:step3.actions"][:, 0])


def test_make_competitive_car_racing_with_weights_equals_a_stand_alone_policy(tmp_path):
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps, seed = 5, 30, 4
    weights = clone_weights()
    g = torch.Generator(device="cuda").manual_seed(3)
    learner = torch.rand((steps, n, 2), generator=g, device="cuda") * 2 - 1
    # the twin: a plain env with the context make_competitive_car_racing builds, car 1 served by a CarPolicy of its own
    twin = crl.HipCarVecEnv(n, seed=seed, frame_stack=4, players=2, done_policy="car0")
    policy = crl.CarPolicy(twin, seed=seed)
    policy.add_network("net", weights, deterministic=True)
    policy.assign(1, "net")
    acts = torch.zeros((n, 2, 2), device="cuda")
    twin.reset()
    recorded = [policy.act(acts)[:, 1].clone()]
    frames = []
    for t in range(steps):
        acts[:, 0] = learner[t]
        buf, rew, done = twin.step_device(acts)
        frames.append((rew[:, 0].clone(), done.clone()))
        recorded.append(policy.act(acts)[:, 1].clone())
    policy.close(), twin.close()
    assert len({r.cpu().numpy().tobytes() for r in recorded}) > steps // 2
    path = tmp_path / "clone.npz"
    np.savez(path, **weights)
    for given in (weights, str(path)):
        a = crl.make_competitive_car_racing(given, seed=seed, num_envs=n)
        assert a.policy is not None and a.drivers is None and a.policy.is_deterministic("opponent")
        assert a.reset().shape == (n, 4, 96, 96)
        assert torch.equal(a._act.view(torch.int32)[:, 1], recorded[0].view(torch.int32))
        for t in range(steps):
            _, ra, da, _ = a.step(learner[t])
            assert torch.equal(a._act.view(torch.int32)[:, 1], recorded[t + 1].view(torch.int32)), t
            assert torch.equal(ra.view(torch.int32).reshape(-1), frames[t][0].view(torch.int32).reshape(-1)), t
        a.close()
    b = crl.make_competitive_car_racing("RULE_BASED", seed=seed, num_envs=2)  # (the names keep their meaning)
    assert b.drivers is not None and b.policy is None
    b.close()

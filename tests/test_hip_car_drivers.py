"""The built-in CarRacing drivers on the device (include/crl.h "car drivers"; csrc/car_driver.hip) against the numpy restatement
``rules.car_driver_reference`` -- tolerance 0 everywhere: open loop on the device's own state through auto-resets, frozen cars and
cars off the track; shards; closed loop against the CPU checker; ``make_competitive_car_racing("RULE_BASED")``; resume; side stream."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
SENTINEL = 7.25  # what an unassigned car's two floats hold before and after ``act``
SOFT = dict(target_speed=30.0, lookahead=7, steer_gain=0.75, epsilon=0.3)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class Tracks:
    """The tile boxes of every env as the device keeps them, re-read (get_track) only for the envs whose episode counter moved"""

    def __init__(self, env):
        from competitive_rl_amd import _native as N

        self.env = env
        self.boxes = np.zeros((env.num_envs, N.CAR_MAX_TILES, 4), F)
        self.n = np.zeros(env.num_envs, np.int64)
        self.episode = np.full(env.num_envs, -1, np.int64)

    def refresh(self, state):
        from competitive_rl_amd.rules import car_tile_boxes

        for i in np.nonzero(state["episode"].astype(np.int64) != self.episode)[0]:
            tr = self.env.get_track(int(i))
            self.n[i] = tr["n"]
            self.boxes[i, :tr["n"]] = car_tile_boxes(tr["tile_poly"])
            self.episode[i] = int(state["episode"][i])


def reference(state, tracks, styles, assign, seed, gid, call, players=2):
    """What ``CarDrivers.act`` must leave in a SENTINEL-filled tensor: styles = {slot: style dict}, assign int [N, players]"""
    from competitive_rl_amd.rules import car_driver_reference

    n = len(state)
    out = np.full((n, players, 2), SENTINEL, F)
    for c in range(players):
        car = state["car"][:, c]
        hull = np.stack([car["hull"][k] for k in ("cx", "cy", "vx", "vy")], axis=1)
        wheels = np.stack([car["wheel"]["cx"], car["wheel"]["cy"]], axis=2)
        for slot, style in styles.items():
            rows = assign[:, c] == slot
            if rows.any():
                a = car_driver_reference(hull, wheels, car["done"], tracks.boxes, tracks.n, style, seed, gid, c, call)
                out[rows, c] = a[rows]
    return out


@pytest.mark.parametrize("n,players", [(1, 2), (3, 2), (3, 1), (65, 2), (130, 2)])
def test_open_loop_actions_equal_the_rule_bit_for_bit(n, players):
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd import rules as R

    base, seed, steps = 1000, 5, 40
    env = crl.HipCarVecEnv(n, seed=11, env_id_base=base, players=players, done_policy="car0" if players == 2 else "any")
    drivers = crl.CarDrivers(env, seed=seed)
    assert drivers.style_names() == ("RANDOM", "RULE_BASED") and drivers.get_style("RULE_BASED") == R.check_car_style()
    assert drivers.set_style("soft", **SOFT) == 2
    styles = {0: dict(kind="RANDOM"), 1: R.check_car_style(), 2: R.check_car_style(**SOFT)}
    idx = np.arange(n)
    assign = np.stack([np.array([1, 2, 0, -1])[idx % 4], np.array([2, -1, 1, 0, 1])[idx % 5]], axis=1)[:, :players].astype(np.int32)
    for c in range(players):
        drivers.assign(c, torch.as_tensor(assign[:, c].copy()).cuda())
    assert np.array_equal(drivers.assignment().cpu().numpy(), assign)
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
    resets = frozen = 0
    for t in range(steps + 1):
        acts.fill_(SENTINEL)
        drivers.act(acts)
        state = env.get_state()
        tracks.refresh(state)
        got, want = acts.cpu().numpy(), reference(state, tracks, styles, assign, seed, gid, t, players)
        bad = np.nonzero((bits(got) != bits(want)).reshape(n, -1).any(1))[0]
        assert len(bad) == 0, ("call", t, "envs", bad[:8], got[bad[:2]], want[bad[:2]])
        assert (got[assign < 0] == SENTINEL).all() and (got[assign >= 0] != SENTINEL).all()
        if players == 2:
            frozen += int(state["car"][far, 1]["done"] == 1)
            if state["car"][far, 1]["done"] == 1 and assign[far, 1] >= 0:
                assert got[far, 1].tolist() == [0.0, 0.0]
        if t == steps:
            break
        a = torch.where(acts == SENTINEL, torch.full_like(acts, 0.1), acts)
        _, _, done = env.step_device(a, render=False)
        resets += int(done.sum())
    assert drivers.calls == steps + 1
    assert resets >= int(soon.sum()) and (tracks.episode[soon] >= 2).all()
    if players == 2:
        assert frozen >= 10
    drivers.close(), env.close()


def test_shards_act_as_the_whole_batch():
    _need_gpu()
    import competitive_rl_amd as crl

    def make(n, base):
        env = crl.HipCarVecEnv(n, seed=21, env_id_base=base)
        d = crl.CarDrivers(env, seed=8)
        d.set_style("soft", **SOFT)
        d.assign(0, "RANDOM"), d.assign(1, "soft")
        env.reset()
        return env, d, torch.zeros((n, 2, 2), device="cuda")

    whole, parts = make(130, 0), [make(65, 0), make(65, 65)]
    for t in range(10):
        for env, d, a in [whole] + parts:
            d.act(a)
        cut = torch.cat([p[2] for p in parts])
        assert torch.equal(whole[2].view(torch.int32), cut.view(torch.int32)), t
        for env, d, a in [whole] + parts:
            env.step_device(a, render=False)
    assert len(torch.unique(whole[2][:, 0, 0])) > 100  # (RANDOM's steer: one draw per env)
    for env, d, a in [whole] + parts:
        d.close(), env.close()


def test_closed_loop_equals_the_cpu_loop():
    """16 envs x 200 steps, both cars RULE_BASED (car 1 with epsilon 0.2), through step_device without a host read inside the loop,
    against oracle.car_oracle.CarBatch driven by rules.car_driver_reference on the same tracks.  The env is bit-exact against the
    CPU checker (tests/test_hip_car_episodes.py), so a difference is the driver's."""
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd import rules as R
    from oracle import car_oracle as co
    from tests.car_scenarios import make_oracle_envs
    from tests.test_hip_car_episodes import batch_to_hip_state

    n, steps, seed = 16, 200, 13
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
    drivers = crl.CarDrivers(env, seed=seed)
    drivers.set_style("eps", epsilon=0.2)
    drivers.assign(0, "RULE_BASED"), drivers.assign(1, "eps")
    styles = [R.check_car_style(), R.check_car_style(epsilon=0.2)]
    acts = torch.zeros((n, 2, 2), device="cuda")
    rec_a = torch.zeros((steps, n, 2, 2), device="cuda")
    rec_r = torch.zeros((steps, n, 2), device="cuda")
    any_done = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    for t in range(steps):  # (device only)
        drivers.act(acts)
        rec_a[t].copy_(acts)
        _, rew, done = env.step_device(acts, render=False)
        rec_r[t].copy_(rew)
        any_done |= done
    got_a, got_r = rec_a.cpu().numpy(), rec_r.cpu().numpy()
    assert not bool(any_done.any()), "an episode ended: the device laid a new track, the CPU loop did not"
    nt = B.E["trk"]["n"].astype(np.int64)
    boxes = B.E["tile_aabb"].copy()
    explored = 0
    for t in range(steps):
        a = np.zeros((n, 2, 2), F)
        for c in range(2):
            car = B.E["car"][:, c]
            hull = np.stack([car["hull"][k] for k in ("cx", "cy", "vx", "vy")], axis=1)
            wheels = np.stack([car["wheel"]["cx"], car["wheel"]["cy"]], axis=2)
            a[:, c] = R.car_driver_reference(hull, wheels, B.E["done"][:, c], boxes, nt, styles[c], seed, np.arange(n), c, t)
        explored += int((R.car_driver_draws(seed, np.arange(n), 1, t)[2] < np.uint64(R.sample_eps_q(0.2))).sum())
        bad = np.nonzero((bits(got_a[t]) != bits(a)).reshape(n, -1).any(1))[0]
        assert len(bad) == 0, ("actions", t, bad, got_a[t][bad[:2]], a[bad[:2]])
        r, _ = B.step(a.astype(np.float64))
        assert np.array_equal(bits(got_r[t]), bits(r.astype(F))), ("rewards", t)
    st = env.get_state()
    assert np.array_equal(st["car"]["tile_visited_count"], B.E["tile_visited_count"])
    # (the run saw both branches, and the cars drove: 4 s at up to 45 units / s over tiles 3.5 units long, from a standing start)
    assert explored > steps * n // 10 and (B.E["tile_visited_count"] > 10).all()
    drivers.close(), env.close()


def test_make_competitive_car_racing_by_name_equals_the_recorded_callable():
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps, seed = 5, 30, 4
    g = torch.Generator(device="cuda").manual_seed(3)
    learner = torch.rand((steps, n, 2), generator=g, device="cuda") * 2 - 1
    # the twin: a plain env with the context make_competitive_car_racing builds, car 1 served by a CarDrivers
    twin = crl.HipCarVecEnv(n, seed=seed, frame_stack=4, players=2, done_policy="car0")
    drivers = crl.CarDrivers(twin, seed=seed)
    drivers.assign(1, "RULE_BASED")
    acts = torch.zeros((n, 2, 2), device="cuda")
    twin.reset()
    recorded = [drivers.act(acts)[:, 1].clone()]
    for t in range(steps):
        acts[:, 0] = learner[t]
        twin.step_device(acts)
        recorded.append(drivers.act(acts)[:, 1].clone())
    drivers.close(), twin.close()
    assert len({r.cpu().numpy().tobytes() for r in recorded}) > steps // 2
    feed = iter(recorded)
    seen = []

    def opponent(obs):
        seen.append(tuple(obs.shape))
        return next(feed)

    a = crl.make_competitive_car_racing("RULE_BASED", seed=seed, num_envs=n)
    b = crl.make_competitive_car_racing(opponent, seed=seed, num_envs=n, batched=True)
    assert a.drivers is not None and b.drivers is None
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob) and oa.shape == (n, 4, 96, 96)
    for t in range(steps):
        oa, ra, da, _ = a.step(learner[t])
        ob, rb, db, _ = b.step(learner[t])
        assert torch.equal(oa, ob) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and torch.equal(da, db), t
        assert torch.equal(a._act.view(torch.int32)[:, 1], recorded[t + 1].view(torch.int32)), t
    assert seen == [(n, 4, 96, 96)] * (steps + 1)
    with pytest.raises(ValueError, match="Unknown car driver style"):
        crl.make_competitive_car_racing("NOBODY", seed=seed, num_envs=2)
    c = crl.make_competitive_car_racing("slow", seed=seed, num_envs=2, styles={"slow": dict(target_speed=10.0)})
    assert c.drivers.get_style("slow")["target_speed"] == 10.0 and c.drivers.assignment().cpu().numpy().tolist() == [[-1, 2], [-1, 2]]
    a.close(), b.close(), c.close()


def test_resume_from_state_dicts_gives_the_uninterrupted_actions():
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps, cut = 6, 30, 10

    def make(driver_seed):
        env = crl.HipCarVecEnv(n, seed=9)
        env.reset()
        return env, crl.CarDrivers(env, seed=driver_seed), torch.zeros((n, 2, 2), device="cuda")

    env, d, acts = make(17)
    d.set_style("soft", **SOFT)
    d.assign(0, "soft")
    d.assign(1, torch.as_tensor(np.array([1, 0, 2, 1, -1, 0], np.int32)).cuda())
    want, saved = [], None
    for t in range(steps):
        if t == cut:
            saved = (env.state_dict(), d.state_dict())
        want.append(d.act(acts).clone())
        _, _, done = env.step_device(acts, render=False)
        assert not bool(done.any())
    d.close(), env.close()
    assert saved[1]["calls"] == cut and saved[1]["seed"] == 17 and set(saved[1]["styles"]) == {"RANDOM", "RULE_BASED", "soft"}
    env, d, acts = make(0)  # (the same tracks: episode 1 of the same seed)
    # a refused load raises ValueError and changes nothing
    before = d.state_dict()
    broken = [dict(saved[1], num_envs=n + 1), dict(saved[1], calls=-1), dict(saved[1], assignment=saved[1]["assignment"][:3]),
              dict(saved[1], styles=dict(saved[1]["styles"], soft=dict(saved[1]["styles"]["soft"], lookahead=99))), dict(saved[1], kind="Policy")]
    for sd in broken:
        with pytest.raises(ValueError, match="load_state_dict"):
            d.load_state_dict(sd)
        after = d.state_dict()
        assert after["styles"] == before["styles"] and after["calls"] == 0 and after["seed"] == 0
        assert np.array_equal(after["assignment"], before["assignment"])
    env.load_state_dict(saved[0])
    d.load_state_dict(saved[1])
    assert d.state_dict()["styles"] == saved[1]["styles"] and d.get_style("soft")["lookahead"] == 7
    for t in range(cut, steps):
        got = d.act(acts)
        assert torch.equal(got.view(torch.int32), want[t].view(torch.int32)), t
        env.step_device(acts, render=False)
    d.close(), env.close()


# ---- side stream: the helper pattern of tests/stream_cases.py (a reference run on the default stream, a held run on a side stream)
DRIVER_STEPS = 10


class CarDriverCase:
    """CarDrivers beside a HipCarVecEnv.  Calls of a pass: DRIVER_STEPS x (act, step_device), an ``assign`` by name after step 3 and an
    ``assign`` by device tensor after step 6.  ``reset()`` and ``set_style`` stay in front of the chain."""
    name = "car-drivers"

    def build(self):
        import competitive_rl_amd as crl

        o = types.SimpleNamespace()
        o.n = 9
        o.env = crl.HipCarVecEnv(o.n, seed=31, done_policy="car0")
        o.drivers = crl.CarDrivers(o.env, seed=2)
        o.drivers.set_style("soft", **SOFT)
        o.drivers.assign(0, "soft"), o.drivers.assign(1, "RULE_BASED")
        o.env.reset()
        st = o.env.get_state()
        st["elapsed"][::2] = 1000 - 7  # auto-resets inside both passes
        st["elapsed"][1::2] = 1000 - DRIVER_STEPS - 4
        o.env.set_state(st)
        o.acts = torch.zeros((o.n, 2, 2), device="cuda")
        o.ids = torch.as_tensor(np.array([0, 1, 2, -1, 2, 1, 0, 2, 1], np.int32)).cuda()
        return o

    def chain(self, rec, o, k):
        with rec.on("A"):
            for t in range(DRIVER_STEPS):
                rec.call("act", o.drivers.act, o.acts)
                rec.keep("step%d.actions" % t, o.acts)
                buf, rew, done = rec.call("step_device", o.env.step_device, o.acts)
                for name, x in (("obs", buf), ("rew", rew), ("done", done)):
                    rec.keep("step%d.%s" % (t, name), x)
                if t == 3:
                    rec.call("assign(name)", o.drivers.assign, 1, "RANDOM" if k else "soft")
                elif t == 6:
                    rec.call("assign(tensor)", o.drivers.assign, 0, o.ids)

    def finish(self, rec, o):
        rec.out["env_state"] = o.env.get_state()
        rec.out["assignment"] = o.drivers.assignment().cpu().numpy()

    def close(self, o):
        o.drivers.close(), o.env.close()


def test_act_and_step_on_a_held_side_stream_equal_the_default_stream():
    _need_gpu()
    from tests import stream_cases as SC

    case = CarDriverCase()
    ref = SC.reference_run(case)
    side = SC.held_run(case, {"A": SC.pick_streams(1)[0]})
    assert SC.same(ref.out, side.out) == []
    dones = [ref.out["%d:step%d.done" % (k, t)] for k in range(2) for t in range(DRIVER_STEPS)]
    assert sum(int(d.sum()) for d in dones) >= 9  # (episodes ended inside the chain)

"""CarLeague on the device (include/crl.h "car league") against its numpy replay (rules.car_league_reference): the books and the
draws on synthetic rewards and done flags over partial wavefronts, two wavefronts and a second block and pools of 1, 5 and 16 agents;
redraw=False, a zero-sum table, shards, PFSP weights; the closed loop on a real env, where a twin env whose car-1 assignments are
written from the HOST out of the replay produces the same actions, rewards and dones bit for bit; resume, refusals, a side stream."""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from competitive_rl_amd import _native as N  # noqa: E402
from competitive_rl_amd import rules as R  # noqa: E402
from tests import car_policy_cases as CP  # noqa: E402

STEPS = 40
A = N.CRL_LEAGUE_MAX_AGENTS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def host(t):
    return t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- synthetic input
def sequence(seed, n, steps=STEPS, p_done=0.3):
    """seeded (steps, n, 2) float32 rewards and done flags with probability 0.3: most wavefronts hold several keys per step"""
    rs = np.random.RandomState(seed)
    rewards = (rs.standard_normal((steps, n, 2)) * 3).astype(np.float32)
    dones = (rs.random_sample((steps, n)) < p_done).astype(np.uint8)
    if n >= 3:  # a NaN and an infinite return: booked as a draw / a win, 0 in the sums
        rewards[3, 1, 0], rewards[5, 2, 0] = np.nan, np.inf
    return rewards, dones


def table(pool, seed=0):
    """non-uniform weights with a zero (a pool of one: its only weight)"""
    w = np.random.RandomState(100 + seed).randint(1, 7, pool).astype(np.uint32)
    if pool >= 2:
        w[1] = 0
    return w


def make(n, pool, seed=4, base=0, players=2):
    """env, policy, drivers and a league whose pool alternates styles and networks: style a // 2 for even a, network a // 2 for odd a"""
    import competitive_rl_amd as crl

    o = types.SimpleNamespace(n=n, seed=seed, base=base)
    o.env = crl.HipCarVecEnv(n, seed=11, env_id_base=base, done_policy="car0" if players == 2 else "any", players=players)
    o.policy = crl.CarPolicy(o.env, seed=12)
    o.drivers = crl.CarDrivers(o.env, seed=13)
    for k in range(pool // 2):
        o.policy.add_network("net%d" % k, CP.random_weights(20 + k), deterministic=bool(k % 2))
    styles = ["RANDOM", "RULE_BASED"] + ["style%d" % k for k in range(2, (pool + 1) // 2)]
    for k, name in enumerate(styles[2:]):
        o.drivers.set_style(name, target_speed=30.0 + k, epsilon=0.1)
    if players == 2:
        o.league = crl.CarLeague(o.env, o.policy, o.drivers, seed=seed)
        for a in range(pool):
            got = o.league.add_style(styles[a // 2]) if a % 2 == 0 else o.league.add_network("net%d" % (a // 2))
            assert got == a
        o.pool = o.league.pool()
        assert len(o.pool) == pool and o.league.agent_names() == tuple(styles[a // 2] if a % 2 == 0 else "net%d" % (a // 2) for a in range(pool))
    return o


def close(o):
    if hasattr(o, "league"):
        o.league.close()
    o.drivers.close(), o.policy.close(), o.env.close()


def column0(n):
    """what the test puts into column 0: (the policy's, the drivers'), both per env"""
    e = np.arange(n)
    return np.where(e % 2 == 0, 0, -1).astype(np.int32), np.where(e % 3 == 0, 1, -1).astype(np.int32)


def assert_served(o, st, col0, where):
    """the three device arrays against the replay's agent array; column 0 as the test put it"""
    net, style = R.car_league_columns(o.pool, st["agent"])
    pa, da = host(o.policy.assignment()), host(o.drivers.assignment())
    assert np.array_equal(host(o.league.assignment()), st["agent"]), where
    assert np.array_equal(pa[:, 1], net) and np.array_equal(da[:, 1], style), where
    assert np.array_equal(pa[:, 0], col0[0]) and np.array_equal(da[:, 0], col0[1]), where


def assert_state(o, st, where=""):
    agent, ret, length, ctr = (host(t) for t in o.league.env_state())
    assert np.array_equal(host(o.league.counters_device()), st["counters"]), where
    assert np.array_equal(agent, st["agent"]) and np.array_equal(length, st["len"]) and np.array_equal(ctr.view(np.uint32), st["draw_ctr"]), where
    nan = np.isnan(st["ret"])
    assert np.array_equal(np.isnan(ret), nan) and np.array_equal(bits(ret)[~nan], bits(st["ret"])[~nan]), where


def play(o, rewards, dones, redraw=True, check=None):
    """the sequence through the league; returns the agent array after every step.  ``check(t)`` runs after step t."""
    rew, don = dev(rewards), dev(dones)
    after = []
    for t in range(len(dones)):
        o.league.step(rew[t], don[t], redraw=redraw)
        after.append(o.league.assignment())
        if check is not None:
            check(t)
    return host(torch.stack(after))


@pytest.mark.parametrize("pool", [1, 5, 16])
@pytest.mark.parametrize("n", [1, 3, 65, 300])
def test_books_and_draws_equal_the_replay_after_every_step(n, pool):
    _need_gpu()
    o = make(n, pool, base=7)
    rewards, dones = sequence(n + pool, n)
    w = table(pool)
    o.league.set_weights(w)
    assert np.array_equal(o.league.weights(), w) and host(o.league.weights_device())[pool:].sum() == 0
    col0 = column0(n)
    o.policy.assign(0, dev(col0[0])), o.drivers.assign(0, dev(col0[1]))
    assert (host(o.league.assignment()) == -1).all()
    o.league.reset_assignment()
    st = R.car_league_draw_all_reference(R.car_league_state(n), pool, w, o.seed, o.base)
    assert_served(o, st, col0, "draw_all")
    box = [st, col0]

    def check(t):
        box[0], _ = R.car_league_reference(box[0], rewards[t:t + 1], dones[t:t + 1], pool, w, o.seed, o.base)
        if t == STEPS // 2:  # column 0 changes mid-sequence: the league's draws in column 1 stay
            flipped = (-col0[0] - 1).astype(np.int32)  # 0 <-> -1
            o.policy.assign(0, dev(flipped)), o.drivers.assign(0, "RANDOM")
            box[1] = (flipped, np.zeros(n, np.int32))  # (RANDOM is style slot 0)
        assert_served(o, box[0], box[1], "step %d" % t)

    after = play(o, rewards, dones, check=check)
    whole, after_ref = R.car_league_reference(st, rewards, dones, pool, w, o.seed, o.base)
    assert np.array_equal(after, after_ref)
    assert_state(o, whole)
    assert whole["counters"][0].sum() == dones.sum() and (pool < 2 or whole["counters"][0, 1] == 0)  # (weight 0: never drawn, never booked)
    c = o.league.counters()
    assert set(c) == set(N.CRL_CAR_LEAGUE_COUNTER_NAMES) | {"win_rate", "mean_return", "mean_opponent_return"}
    played = c["episodes"] > 0
    assert len(c["episodes"]) == pool and np.isnan(c["win_rate"][~played]).all()
    assert np.array_equal(c["win_rate"][played], (c["wins"][played] + 0.5 * c["draws"][played]) / c["episodes"][played])
    assert np.array_equal(c["mean_return"][played], c["return_sum"][played] / 256.0 / c["episodes"][played])
    assert np.array_equal(c["mean_opponent_return"][played], c["opponent_return_sum"][played] / 256.0 / c["episodes"][played])
    close(o)


def test_redraw_false_books_results_and_keeps_assignments_and_draw_counters():
    _need_gpu()
    n, pool = 65, 5
    o = make(n, pool)
    rewards, dones = sequence(1, n, 12)
    w = table(pool)
    o.league.set_weights(w)
    o.league.reset_assignment()
    st = R.car_league_draw_all_reference(R.car_league_state(n), pool, w, o.seed, o.base)
    after = play(o, rewards, dones, redraw=False)
    ref, _ = R.car_league_reference(st, rewards, dones, pool, w, o.seed, o.base, redraw=False)
    assert (after == st["agent"]).all() and (ref["draw_ctr"] == 1).all() and ref["counters"][0].sum() == dones.sum() > 0
    assert_state(o, ref)
    # reset_agent: one column; reset: everything but key, table, draw counters and assignments
    o.league.reset_agent(o.league.agent_names()[2])
    assert_state(o, R.car_league_reset_agent_reference(ref, 2))
    o.league.reset()
    fresh = R.car_league_state(n)
    assert_state(o, dict(fresh, agent=ref["agent"], draw_ctr=ref["draw_ctr"]))
    # seed: a new key, the draw counters start over
    o.league.seed(99)
    o.league.reset_assignment()
    assert_state(o, R.car_league_draw_all_reference(fresh, pool, w, 99, o.base))
    close(o)


def test_a_zero_sum_table_keeps_assignments_and_draw_counters():
    _need_gpu()
    n, pool = 65, 5
    o = make(n, pool)
    rewards, dones = sequence(2, n, 12)
    o.league.reset_assignment()  # (weight 1 each)
    st = R.car_league_draw_all_reference(R.car_league_state(n), pool, [1] * pool, o.seed, o.base)
    # p = 0.5 for an agent never played, 0.5 ** 64 * 65535 < 1 and floor 0: every weight is 0 (set_weights would refuse such a table)
    o.league.pfsp_weights("hard", 64, 0)
    assert not o.league.weights().any()
    after = play(o, rewards, dones)
    ref, _ = R.car_league_reference(st, rewards, dones, pool, [0] * pool, o.seed, o.base)
    assert (after == st["agent"]).all() and (ref["draw_ctr"] == 1).all() and ref["counters"][0].sum() == dones.sum() > 0
    assert_state(o, ref)
    net, style = R.car_league_columns(o.pool, st["agent"])
    assert np.array_equal(host(o.policy.assignment())[:, 1], net) and np.array_equal(host(o.drivers.assignment())[:, 1], style)
    close(o)


def test_shards_with_the_same_table_draw_what_the_whole_batch_draws():
    _need_gpu()
    pool = 5
    rewards, dones = sequence(3, 5, 20, p_done=0.5)
    w = table(pool)
    whole, lo, hi = make(5, pool), make(3, pool, base=0), make(2, pool, base=3)
    parts = ((whole, slice(0, 5)), (lo, slice(0, 3)), (hi, slice(3, 5)))
    after = {}
    for o, cut in parts:
        o.league.set_weights(w)
        o.league.reset_assignment()
        first = host(o.league.assignment())
        after[id(o)] = np.concatenate([first[None], play(o, rewards[:, cut], dones[:, cut])])
    assert np.array_equal(np.concatenate([after[id(lo)], after[id(hi)]], axis=1), after[id(whole)])
    assert np.array_equal(host(lo.league.counters_device()) + host(hi.league.counters_device()), host(whole.league.counters_device()))
    assert len(np.unique(after[id(whole)])) >= 3 and dones.sum() >= 30
    for o, _ in parts:
        close(o)


def test_pfsp_weights_equal_the_reference_fed_the_leagues_planes():
    _need_gpu()
    import competitive_rl_amd as crl

    n, pool = 65, 5
    o = make(n, pool)
    rewards, dones = sequence(4, n, 20)
    o.league.reset_assignment()
    play(o, rewards, dones)
    planes = host(o.league.counters_device())
    assert (planes[0, :pool] > 0).all()
    ledger_order = [0, 1, 2, 3, 4, 6]  # pfsp_weights_reference takes the ledger's six planes: it reads episodes, wins, draws
    other = planes * 3
    other[0] += np.arange(A)  # (more episodes than results: still a table wins + draws / 2 <= episodes)
    for mode, k, floor in (("hard", 3, 2), ("variance", 1, 0), ("hard", 1, 1)):
        o.league.pfsp_weights(mode, k, floor)
        assert np.array_equal(host(o.league.weights_device()), crl.pfsp_weights_reference(planes[ledger_order], pool, mode, k, floor))
        o.league.pfsp_weights(mode, k, floor, counters=dev(other))
        assert np.array_equal(host(o.league.weights_device()), crl.pfsp_weights_reference(other[ledger_order], pool, mode, k, floor))
    assert len(np.unique(o.league.weights())) > 1
    with pytest.raises(ValueError):
        o.league.pfsp_weights("soft")
    with pytest.raises(ValueError):
        o.league.pfsp_weights("hard", 2, 1, counters=dev(other[:6]))
    with pytest.raises(N.CrlError):
        o.league.pfsp_weights("hard", 0, 1)
    close(o)


# ---------------------------------------------------------------------------------------------------------------- the closed loop
LOOP_N, LOOP_STEPS, LOOP_W = 65, 14, np.array([2, 1, 3, 2], np.uint32)


def build_loop(league=True, first_done=2):
    """65 envs on their first episode with ``elapsed`` staggered just below 1000: every env's episode ends inside about 12 steps.
    The pool: RANDOM, RULE_BASED, a sampling network and a deterministic one.  Car 0: the sampling network in even envs, RULE_BASED in
    odd ones."""
    import competitive_rl_amd as crl

    o = types.SimpleNamespace()
    o.env = crl.HipCarVecEnv(LOOP_N, seed=21, done_policy="car0")
    o.policy = crl.CarPolicy(o.env, seed=22)
    o.drivers = crl.CarDrivers(o.env, seed=23)
    o.policy.add_network("sampler", CP.random_weights(31, 2.0))
    o.policy.add_network("greedy", CP.random_weights(32, 2.0), deterministic=True)
    e = np.arange(LOOP_N)
    o.col0 = (np.where(e % 2 == 0, 0, -1).astype(np.int32), np.where(e % 2 == 1, 1, -1).astype(np.int32))
    o.policy.assign(0, dev(o.col0[0])), o.drivers.assign(0, dev(o.col0[1]))
    o.env.reset()
    st = o.env.get_state()
    st["elapsed"][:] = 1000 - first_done - e % 10
    o.env.set_state(st)
    o.acts = torch.zeros((LOOP_N, 2, 2), device="cuda")
    if league:
        o.league = crl.CarLeague(o.env, o.policy, o.drivers, seed=24)
        for name in ("RANDOM", "RULE_BASED"):
            o.league.add_style(name)
        for name in ("sampler", "greedy"):
            o.league.add_network(name)
        o.league.set_weights(LOOP_W)
        o.pool = o.league.pool()
    return o


def loop(o, steps, before_step=lambda t: None):
    """drivers.act; policy.act; step_device(render=False); league.step -- recording actions, rewards, dones and the agent array"""
    out = dict(actions=[], rewards=[], dones=[], agents=[])
    for t in range(steps):
        before_step(t)
        o.drivers.act(o.acts), o.policy.act(o.acts)
        out["actions"].append(o.acts.clone())
        _, rew, done = o.env.step_device(o.acts, render=False)
        out["rewards"].append(rew.clone()), out["dones"].append(done.clone())
        if hasattr(o, "league"):
            o.league.step(rew, done)
            out["agents"].append(o.league.assignment())
    return {k: host(torch.stack(v)) if v else None for k, v in out.items()}


def test_closed_loop_serves_the_drawn_opponent_from_the_first_step_of_the_new_episode():
    _need_gpu()
    a = build_loop()
    a.league.reset_assignment()
    got = loop(a, LOOP_STEPS)
    st0 = R.car_league_draw_all_reference(R.car_league_state(LOOP_N), 4, LOOP_W, 24)
    ref, after = R.car_league_reference(st0, got["rewards"], got["dones"], 4, LOOP_W, 24)
    assert np.array_equal(got["agents"], after)
    assert_state(a, ref)
    assert got["dones"].sum() == LOOP_N and got["dones"][:12].sum() >= LOOP_N - 6  # every env's first episode ended, most of them early
    assert ref["counters"][0].sum() == LOOP_N and (ref["counters"][0, :4] > 0).all() and (after[-1] != st0["agent"]).sum() >= LOOP_N // 3
    close(a)
    # the twin: no league; car 1's assignments written from the host out of the replay before every step
    b = build_loop(league=False)
    agents = np.concatenate([st0["agent"][None], after])

    def assign_from_host(t):
        net, style = R.car_league_columns(a.pool, agents[t])
        b.policy.assign(1, dev(net)), b.drivers.assign(1, dev(style))

    twin = loop(b, LOOP_STEPS, assign_from_host)
    for k in ("actions", "rewards"):
        assert np.array_equal(bits(twin[k]), bits(got[k])), k
    assert np.array_equal(twin["dones"], got["dones"])
    assert np.array_equal(host(b.policy.assignment())[:, 0], b.col0[0]) and np.array_equal(host(b.drivers.assignment())[:, 0], b.col0[1])
    # ... and the draw matters: with the opponents of the first episode kept, the run differs once episodes have ended
    c = build_loop(league=False)
    net, style = R.car_league_columns(a.pool, st0["agent"])
    c.policy.assign(1, dev(net)), c.drivers.assign(1, dev(style))
    kept = loop(c, LOOP_STEPS)
    assert not np.array_equal(bits(kept["actions"]), bits(got["actions"]))
    close(b), close(c)


def test_resume_mid_run_continues_bit_for_bit():
    _need_gpu()
    # (the env's state dict does not hold the tracks, a function of (seed, env id, episode): the checkpoint is taken while every env is
    # on its first episode; the auto-resets, the books' entries and the redraws all fall behind it)
    head, tail = 3, 12
    a = build_loop(first_done=head + 1)
    a.league.reset_assignment()
    first = loop(a, head)
    assert first["dones"].sum() == 0
    saved = dict(env=a.env.state_dict(), policy=a.policy.state_dict(), drivers=a.drivers.state_dict(), league=a.league.state_dict())
    assert saved["league"]["ret"].any() and (saved["league"]["len"] == head).all() and (saved["league"]["draw_ctr"] == 1).all()
    want = loop(a, tail)
    want_state = a.league.state_dict()
    assert want["dones"].sum() == LOOP_N and want_state["counters"][0].sum() == LOOP_N
    close(a)
    import competitive_rl_amd as crl

    b = types.SimpleNamespace()
    b.env = crl.HipCarVecEnv(LOOP_N, seed=21, done_policy="car0")
    b.policy, b.drivers = crl.CarPolicy(b.env, seed=0), crl.CarDrivers(b.env, seed=0)
    b.league = crl.CarLeague(b.env, b.policy, b.drivers, seed=0)
    b.env.reset()
    b.env.load_state_dict(saved["env"]), b.policy.load_state_dict(saved["policy"]), b.drivers.load_state_dict(saved["drivers"])
    b.league.load_state_dict(saved["league"])
    assert b.league.agent_names() == ("RANDOM", "RULE_BASED", "sampler", "greedy") and np.array_equal(b.league.weights(), LOOP_W)
    b.acts = torch.zeros((LOOP_N, 2, 2), device="cuda")
    got = loop(b, tail)
    for k in ("actions", "rewards"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["dones"], want["dones"]) and np.array_equal(got["agents"], want["agents"])
    got_state = b.league.state_dict()
    assert sorted(got_state) == sorted(want_state)
    for k, v in want_state.items():
        assert (np.asarray(v).tobytes() == np.asarray(got_state[k]).tobytes()) if isinstance(v, np.ndarray) else got_state[k] == v, k
    close(b)


def _same_dict(x, y):
    return sorted(x) == sorted(y) and all((np.asarray(v).tobytes() == np.asarray(y[k]).tobytes()) if isinstance(v, np.ndarray) else y[k] == v
                                          for k, v in x.items())


def test_a_tampered_state_dict_is_refused_and_changes_nothing():
    _need_gpu()
    import copy

    n, pool = 9, 5
    o = make(n, pool)
    rewards, dones = sequence(5, n, 10)
    o.league.set_weights(table(pool))
    o.league.reset_assignment()
    play(o, rewards, dones)
    good = o.league.state_dict()
    assert good["counters"][0].sum() == dones.sum() > 0 and good["kind"] == "CarLeague"
    other = make(n, pool, seed=77)
    other.league.reset_assignment()
    before = other.league.state_dict()
    assign_before = host(other.policy.assignment()), host(other.drivers.assignment())
    tampered = []
    for change in ("num_envs", "network", "slot", "kind", "agent", "weights", "counters", "prefix"):
        sd = copy.deepcopy(good)
        if change == "num_envs":
            sd["num_envs"] = n + 1
        elif change == "network":
            sd["pool"][1]["name"] = "nobody"
        elif change == "slot":
            sd["pool"][3]["slot"] = 0
        elif change == "kind":
            sd["kind"] = "CarPolicy"
        elif change == "agent":
            sd["agent"][0] = pool
        elif change == "weights":
            sd["weights"] = np.zeros(pool, np.uint32)
        elif change == "counters":
            sd["counters"] = sd["counters"][:6]
        else:
            sd["pool"][0], sd["pool"][2] = sd["pool"][2], sd["pool"][0]
        tampered.append(sd)
    for sd in tampered:
        with pytest.raises(ValueError, match="load_state_dict"):
            other.league.load_state_dict(sd)
        assert _same_dict(other.league.state_dict(), before)
        assert np.array_equal(host(other.policy.assignment()), assign_before[0]) and np.array_equal(host(other.drivers.assignment()), assign_before[1])
    # the untampered one loads, into a league with the same pool and into one whose pool is still empty; car 1's columns follow
    import competitive_rl_amd as crl

    other.league.load_state_dict(good)
    empty = crl.CarLeague(other.env, other.policy, other.drivers, seed=1)
    empty.load_state_dict(good)
    for lg in (other.league, empty):
        assert _same_dict(lg.state_dict(), good)
    net, style = R.car_league_columns(o.pool, good["agent"])
    assert np.array_equal(host(other.policy.assignment())[:, 1], net) and np.array_equal(host(other.drivers.assignment())[:, 1], style)
    empty.close()
    close(o), close(other)


def test_refusals():
    _need_gpu()
    import competitive_rl_amd as crl

    one = make(4, 2, players=1)
    with pytest.raises(N.CrlError, match="two-car"):
        crl.CarLeague(one.env, one.policy, one.drivers)
    close(one)
    o = make(4, 16)
    o.drivers.set_style("extra", target_speed=20.0)
    with pytest.raises(ValueError, match="16"):
        o.league.add_style("extra")
    h = C.c_int32(-5)
    assert o.league._L.crl_car_league_add_agent(o.league._h, N.CRL_CAR_LEAGUE_STYLE, 0, C.byref(h), None) == -1 and h.value == -5
    assert b"16" in o.league._L.crl_last_error()
    close(o)
    o = make(4, 2)
    other = make(4, 2)
    with pytest.raises(ValueError, match="belong"):
        crl.CarLeague(o.env, other.policy, o.drivers)
    close(other)
    for bad in (lambda: o.league.add_network("nobody"), lambda: o.league.add_style("nobody"), lambda: o.league.add_style("RANDOM"),
                lambda: o.league.reset_agent("nobody"), lambda: o.league.set_weights([1, 2, 3]), lambda: o.league.set_weights([0, 0])):
        with pytest.raises((ValueError, N.CrlError)):
            bad()
    lib, hdl = o.league._L, o.league._h
    assert lib.crl_car_league_add_agent(hdl, 2, 0, None, None) == -1 and lib.crl_car_league_add_agent(hdl, N.CRL_CAR_LEAGUE_NETWORK, 8, None, None) == -1
    assert lib.crl_car_league_add_agent(hdl, N.CRL_CAR_LEAGUE_STYLE, 16, None, None) == -1 and lib.crl_car_league_reset_agent(hdl, 2, None) == -1
    assert lib.crl_car_league_step(hdl, None, None, 1, None) == -1 and lib.crl_car_league_step(None, None, None, 1, None) == -1
    rew, done = torch.zeros((4, 2), device="cuda"), torch.zeros((4,), dtype=torch.uint8, device="cuda")
    o.league.step(rew, done)
    for r, d in ((rew.double(), done), (rew, done.bool()), (rew, done.to(torch.int32)), (rew[:3], done), (rew, done[:3]), (rew[:, :1], done),
                 (torch.zeros((4, 4), device="cuda")[:, ::2], done), (rew.cpu(), done), (rew, done.cpu()), (host(rew), host(done)),
                 (torch.zeros((4,), device="cuda"), done)):
        with pytest.raises((TypeError, ValueError)):
            o.league.step(r, d)
    assert o.league.agents == 2 and host(o.league.env_state()[2]).tolist() == [1, 1, 1, 1]  # only the good step counted
    close(o)


def test_the_sequence_on_a_side_stream_gives_the_bits_of_the_default_stream():
    _need_gpu()
    n, pool = 300, 5
    rewards, dones = sequence(6, n)
    w = table(pool)
    out = []
    for stream in (None, torch.cuda.Stream()):
        o = make(n, pool)
        rew, don = dev(rewards), dev(dones)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            o.league.set_weights(w)
            o.league.reset_assignment()
            after = [o.league.assignment()]
            for t in range(STEPS):
                o.league.step(rew[t], don[t])
                after.append(o.league.assignment())
                if t == STEPS // 2:
                    o.league.pfsp_weights("hard", 2, 1)
            kept = [torch.stack(after), o.league.counters_device(), o.league.weights_device(), o.policy.assignment(), o.drivers.assignment()]
            kept += list(o.league.env_state())
        torch.cuda.synchronize()
        out.append([host(t).tobytes() for t in kept])
        close(o)
    assert out[0] == out[1]

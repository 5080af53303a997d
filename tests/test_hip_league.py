"""LeagueEnvWrapper (competitive_rl_amd/league.py, csrc/pong_league.hip) on the device: per-env opponents against the existing
single-opponent wrapper, the shared frame history, the written draw rule (restated in tests/test_league_rules.py), and the hot loop's
freedom from host work.  Everything is bytes or integers: tolerance 0 throughout."""
import time

import numpy as np
import pytest
import torch

from competitive_rl_amd.league import LeagueEnvWrapper
from tests.test_league_rules import DOMAIN_ACTION, DOMAIN_OPPONENT, league_draw

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _env(n, seed, base=0):
    import competitive_rl_amd as crl

    return crl.make_envs("cPongDouble-v0", num_envs=n, log_dir=None, seed=seed, resized_dim=42, frame_stack=None, env_id_base=base)


def _near_the_end(env, first_id=0):
    """Episodes end soon and not all at once: env with global id g starts 1 + g % 4 rounds before the end of its episode (scores 19-20 and
    below; the existing stack tests put `num_rounds` to 20 the same way)."""
    st = env.get_state()
    g = first_id + np.arange(len(st))
    st["num_rounds"] = 20 - g % 4
    env.set_state(st)


def _learner_actions(steps, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 3, (steps, n), generator=g, device="cuda", dtype=torch.int32)


def _with_logits(tour, name):
    """The tournament wrapper asks its policy for actions only; the comparison wants the logits too."""
    pol = tour.agents[name]
    plain = pol.act_device
    pol.act_device = lambda obs, out=None: plain(obs, out=out, want_logits=True)
    return pol


def _fixed_assignment_run(n, steps, assign, sample=None, seed=21):
    """A league with the fixed assignment `assign` over [RULE_BASED, WEAK, MEDIUM] beside one TournamentEnvWrapper per agent on identically
    seeded envs, the same learner actions: for every agent, the envs assigned to it must show identical observations (both views), rewards,
    dones, opponent actions and logits at every step.  Mismatches are counted on the device; returns (mismatches, steps with a done)."""
    import competitive_rl_amd as crl

    names = ["RULE_BASED", "WEAK", "MEDIUM"]
    lg = LeagueEnvWrapper(_env(n, seed), n, names, seed=5)
    lg.record_logits = True
    tours = [crl.TournamentEnvWrapper(_env(n, seed), n, names) for _ in names]
    dev = lg.device
    assign = torch.as_tensor(assign, dtype=torch.int32, device=dev)
    pick = torch.arange(n, device=dev) if sample is None else torch.as_tensor(sample, device=dev)
    rows = [pick[assign[pick] == a] for a in range(3)]
    first = lg.reset()
    for a, tw in enumerate(tours):
        tw.reset_opponent(names[a])
        assert torch.equal(tw.reset(), first)
        _near_the_end(tw.env)
    _near_the_end(lg.env)
    lg.set_opponents(assign)
    pols = [None, _with_logits(tours[1], "WEAK"), _with_logits(tours[2], "MEDIUM")]
    acts = _learner_actions(steps, n, 3)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    waves = torch.zeros((), dtype=torch.int64, device=dev)
    for t in range(steps):
        buf, rew, done = lg.step_device(acts[t])
        waves += done.any()
        for a, tw in enumerate(tours):
            tbuf, trew, tdone = tw.step_device(acts[t])
            r = rows[a]
            bad += (buf[r] != tbuf[r]).any() + (rew[r] != trew[r]).any() + (done[r] != tdone[r]).any() + (lg._act[r] != tw._act[r]).any()
            if pols[a] is not None:
                bad += (lg.logits()[r] != pols[a].logits()[r]).any()
    out = int(bad), int(waves)
    assert np.array_equal(lg.counts(), np.bincount(assign.cpu().numpy(), minlength=3))
    lg.close()
    for tw in tours:
        tw.close()
    return out


@pytest.mark.parametrize("shuffled", [False, True])
def test_fixed_assignment_equals_the_single_opponent_wrapper(shuffled):
    _need_gpu()
    n, steps = 1003, 2000  # ragged on purpose: not a multiple of 8 or 64
    assign = np.arange(n) % 3
    if shuffled:
        assign = np.random.RandomState(4).permutation(assign)
    bad, waves = _fixed_assignment_run(n, steps, assign)
    print("fixed assignment: n", n, "steps", steps, "mismatching comparisons", bad, "steps with an episode end", waves)
    assert waves >= 3, "the run must contain several waves of episode ends"
    assert bad == 0


@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])
def test_fixed_assignment_at_the_group_edges(n):
    _need_gpu()
    bad, waves = _fixed_assignment_run(n, 400, (np.arange(n) + 1) % 3)
    print("group edges: n", n, "mismatching comparisons", bad, "steps with an episode end", waves)
    assert bad == 0


def test_fixed_assignment_at_65536_envs_on_512_sampled_envs():
    _need_gpu()
    n = 65536
    rs = np.random.RandomState(6)
    bad, waves = _fixed_assignment_run(n, 150, rs.randint(0, 3, n), sample=np.sort(rs.choice(n, 512, replace=False)))
    print("65 536 envs: mismatching comparisons", bad, "steps with an episode end", waves)
    assert bad == 0 and waves >= 3


def test_all_on_one_agent_equals_the_policy_launch():
    """Every env on MEDIUM: the list launch must give what Policy.act_device (the launch without a list) gives for the same frames --
    actions and logits, while the ring wraps three times."""
    _need_gpu()
    import competitive_rl_amd as crl

    n = 1003
    lg = LeagueEnvWrapper(_env(n, 1), n, ["RULE_BASED", "MEDIUM", "WEAK"])
    lg.record_logits = True
    pol = crl.get_compute_action_function("MEDIUM", n, lg.device)
    lg.set_opponents("MEDIUM")
    assert lg.counts().tolist() == [0, n, 0] and np.array_equal(lg.agent_lists()["MEDIUM"], np.arange(n)) and len(lg.agent_lists()["WEAK"]) == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    mine = torch.zeros((n,), dtype=torch.int32, device=lg.device)
    for t in range(12):
        f = torch.randint(0, 256, (n, 1, 42, 42), generator=g, device="cuda", dtype=torch.uint8) * (torch.rand((n, 1, 42, 42), generator=g, device="cuda") > 0.7)
        lg.prev_opponent_obs = f
        a = lg._fill_actions(mine)[:, 1].clone()
        b = pol.act_device(f, want_logits=True)
        assert torch.equal(a, b) and torch.equal(lg.logits(), pol.logits()), t
    assert torch.equal(lg.get_stack(), pol.get_stack())
    pol.close(), lg.close()


def _stack_of(frames):
    return torch.stack([f[:, 0] for f in frames[-4:]], 1).contiguous()


def test_a_switched_env_is_judged_on_the_frames_it_showed():
    """Envs on RULE_BASED for >= 4 steps are switched to WEAK: the next opponent action is Policy.compute_action on the four opponent-view
    observations the test recorded itself -- in mid-episode, and right after an episode end (the history is not cleared there)."""
    _need_gpu()
    import competitive_rl_amd as crl

    n = 40
    lg = LeagueEnvWrapper(_env(n, 8), n, ["RULE_BASED", "WEAK"])
    lg.record_logits = True
    weak = crl.get_compute_action_function("WEAK", n, lg.device)
    lg.reset()
    acts = _learner_actions(1200, n, 9)
    shown = [lg.prev_opponent_obs.clone()]
    for t in range(6):
        buf, _, _ = lg.step_device(acts[t])
        shown.append(buf[:, 1].clone())
    half = torch.arange(n, device=lg.device) % 2 == 0
    lg.set_opponents(half.to(torch.int32))
    expect = weak.compute_action(_stack_of(shown)).reshape(-1)
    expect_logits = weak.logits().clone()
    lg.step_device(acts[6])
    got = lg._act[:, 1].to(torch.int64)
    assert torch.equal(got[half], expect[half]) and bool((got[~half] == 999).all())
    assert torch.equal(lg.logits()[half], expect_logits[half])
    # at an episode end
    lg.set_opponents("RULE_BASED")
    _near_the_end(lg.env)
    shown, ended, t = [lg.prev_opponent_obs.clone()], None, 7
    while t < 1200:
        buf, _, done = lg.step_device(acts[t])
        shown.append(buf[:, 1].clone())
        t += 1
        if len(shown) >= 5 and bool(done.any()):
            ended = done.bool().clone()
            break
    assert ended is not None, "no episode ended"
    lg.set_opponents(ended.to(torch.int32))
    expect = weak.compute_action(_stack_of(shown)).reshape(-1)
    lg.step_device(acts[t])
    got = lg._act[:, 1].to(torch.int64)
    assert torch.equal(got[ended], expect[ended]) and bool((got[~ended] == 999).all())
    assert bool((_stack_of(shown)[ended][:, :3] != 0).any()), "the frames before the episode end are part of the history"
    with pytest.raises(ValueError, match="full-size ActorCritic is not"):
        from competitive_rl_amd import spaces
        from competitive_rl_amd.policy_serving import Policy
        lg.add_agent("BIG", Policy(spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3), n, use_light_model=False, device=lg.device))
    weak.close(), lg.close()


NAMES4 = ["RANDOM", "WEAK", "MEDIUM", "RULE_BASED"]


def _drawn_run(n, base, steps, acts, seed=5, league_seed=77, explicit=False, total=None):
    """A league over all four agents with one draw per env at the start and a fresh one at every episode end.  explicit=False: the
    league does it (resample_on_done); every step's RANDOM actions, assignment, counts and lists are checked against the numpy rule.
    explicit=True: resample_on_done is off and the test itself calls set_opponents with what the rule and the done flags give.
    Returns per-step records (checksums of both views, rewards, dones, opponent actions, assignment)."""
    lg = LeagueEnvWrapper(_env(n, seed, base), n, NAMES4, seed=league_seed, resample_on_done=not explicit)
    assert lg.env_id_base == base
    gid = base + np.arange(n)
    lg.reset()
    _near_the_end(lg.env, base)
    ctr = np.zeros(n, np.int64)
    expect = league_draw(league_seed, gid, ctr, DOMAIN_OPPONENT, 4)
    ctr += 1
    if explicit:
        lg.set_opponents(expect)
    else:
        lg.reset_opponent()
    assert np.array_equal(lg.assignment.cpu().numpy(), expect)
    w = torch.arange(1, 2 * 42 * 42 + 1, device=lg.device, dtype=torch.int64)
    rec, changed_total = [], 0
    for t in range(steps):
        before = expect
        buf, rew, done = lg.step_device(acts[t])
        opp = lg._act[:, 1].cpu().numpy()
        d = done.cpu().numpy().astype(bool)
        is_random = before == NAMES4.index("RANDOM")
        assert np.array_equal(opp[is_random], league_draw(league_seed, gid, t, DOMAIN_ACTION, 3)[is_random]), t
        assert (opp[before == NAMES4.index("RULE_BASED")] == 999).all() and np.isin(opp[(before == 1) | (before == 2)], (0, 1, 2)).all()
        expect = np.where(d, league_draw(league_seed, gid, ctr, DOMAIN_OPPONENT, 4), before)
        ctr += d
        if explicit:
            if d.any():
                lg.set_opponents(expect)
        else:
            now = lg.assignment.cpu().numpy()
            assert np.array_equal(now, expect), t
            assert (now[~d] == before[~d]).all()  # the assignment changes only where `done` was set
            changed_total += int((now != before).sum())
            if d.any() or t % 50 == 0:
                counts, lists = lg.counts(), lg.agent_lists()
                assert counts.sum() == n and np.array_equal(counts, np.bincount(now, minlength=4))
                assert sorted(lists) == ["MEDIUM", "WEAK"]
                for name, idx in lists.items():
                    assert np.array_equal(idx, np.flatnonzero(now == NAMES4.index(name))), (t, name)
        rec.append(((buf.view(n, -1).to(torch.int64) * w).sum(1).cpu().numpy(), rew.cpu().numpy().copy(), d, opp, expect))
    lg.close()
    if not explicit:
        assert changed_total > 0
    return rec


def _same_records(a, b):
    for t, (x, y) in enumerate(zip(a, b)):
        for k, what in enumerate(("frames", "rewards", "dones", "opponent actions", "assignment")):
            assert np.array_equal(x[k], y[k]), (t, what)


def _joined(lo, hi):
    return [tuple(np.concatenate([x[k], y[k]]) for k in range(5)) for x, y in zip(lo, hi)]


def test_random_actions_and_redraws_follow_the_written_rule_and_do_not_depend_on_sharding():
    _need_gpu()
    n, steps = 1000, 700
    acts = _learner_actions(steps, n, 13)
    whole = _drawn_run(n, 0, steps, acts)
    ends = sum(int(r[2].sum()) for r in whole)
    print("drawn run: episode ends", ends, "steps with an end", sum(bool(r[2].any()) for r in whole))
    assert ends >= n // 4  # (the quarter of the envs that started one round before the end, at the least)
    final = whole[-1][4]
    assert len(set(final.tolist())) == 4
    lo = _drawn_run(n // 2, 0, steps, acts[:, :n // 2])
    hi = _drawn_run(n // 2, n // 2, steps, acts[:, n // 2:])
    _same_records(_joined(lo, hi), whole)


def test_resample_on_done_equals_explicit_set_opponents_calls():
    _need_gpu()
    n, steps = 520, 600
    acts = _learner_actions(steps, n, 14)
    _same_records(_drawn_run(n, 0, steps, acts, explicit=True), _drawn_run(n, 0, steps, acts))


def test_frame_stack_bound_through_the_league_equals_the_generic_update():
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps = 96, 200
    a = LeagueEnvWrapper(_env(n, 2), n, NAMES4, seed=3, resample_on_done=True)
    b = LeagueEnvWrapper(_env(n, 2), n, NAMES4, seed=3, resample_on_done=True)
    dev = a.device
    f1, f2 = crl.FrameStackTensor(n, (1, 42, 42), 4, dev), crl.FrameStackTensor(n, (1, 42, 42), 4, dev)
    f2._bind_tried = True  # stays on the generic kernel
    f1.update(a.reset()), f2.update(b.reset())
    _near_the_end(a.env), _near_the_end(b.env)
    a.reset_opponent(), b.reset_opponent()
    books = [dict(ep=torch.zeros((n, 1), dtype=torch.float32, device=dev), rr=[], lr=[], steps=0, episodes=0) for _ in range(2)]
    acts = _learner_actions(steps, n, 15)
    for t in range(steps):
        for env, f, bk in ((a, f1, books[0]), (b, f2, books[1])):
            out = crl.step_envs(acts[t], env, bk["ep"], f, bk["rr"], bk["lr"], bk["steps"], bk["episodes"], dev, False)
            bk["episodes"], bk["steps"] = out[5], out[6]
        assert torch.equal(f1.get(), f2.get()), t
    assert f1.fused_updates > 0 and books[0]["episodes"] == books[1]["episodes"] > 0
    assert torch.equal(a.assignment, b.assignment)
    a.close(), b.close()


def test_step_device_does_no_host_work():
    """50 league steps (mixed pool, resample_on_done, learner actions produced on the device) enqueued behind a long-running launch: a
    device-to-host copy or a synchronisation anywhere in them would have to wait for that launch, so the host must be through with all
    50 calls while the launch still runs.  No graph is captured."""
    _need_gpu()
    n = 4096
    lg = LeagueEnvWrapper(_env(n, 3), n, NAMES4, seed=1, resample_on_done=True)
    lg.reset()
    _near_the_end(lg.env)
    lg.reset_opponent()
    acts = _learner_actions(60, n, 16)
    for t in range(10):  # warm-up: lazy allocations, kernel loading
        lg.step_device(acts[t])
    x = torch.randn((8192, 8192), device=lg.device)
    y = torch.empty_like(x)
    torch.mm(x, x, out=y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.mm(x, x, out=y)
    torch.cuda.synchronize()
    reps = int(max(8, min(400, 1.5 / (time.perf_counter() - t0))))  # about 1.5 s of queued work
    for _ in range(reps):
        torch.mm(x, x, out=y)
    busy = torch.cuda.Event()
    busy.record()
    t0 = time.perf_counter()
    for t in range(10, 60):
        prev = lg.step_device(acts[t] if t % 2 else (acts[t] + 1) % 3)  # (the second form is computed on the device)
    host = time.perf_counter() - t0
    still_busy = not busy.query()
    torch.cuda.synchronize()
    print("50 step_device calls took the host", round(host * 1e3, 2), "ms behind", reps, "queued matrix products; device still busy:", still_busy)
    assert still_busy, "the host waited for the device inside step_device"
    assert prev[0].shape == (n, 2, 1, 42, 42)
    lg.close()

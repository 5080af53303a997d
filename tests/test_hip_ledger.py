"""LeagueLedger (competitive_rl_amd/ledger.py, csrc/pong_ledger.hip) on the device: the books against a numpy replay of the recorded
steps, the weighted redraws against the written rule (restated in tests/test_ledger_rules.py), the PFSP weight kernel against its numpy
restatement, sharding, checkpoints, and the hot loop's freedom from host work.  Everything is integers or float64 with one rounding per
operation: tolerance 0 throughout."""
import time

import numpy as np
import pytest
import torch

from competitive_rl_amd import _native as N
from competitive_rl_amd.league import LeagueEnvWrapper
from competitive_rl_amd.ledger import LeagueLedger, ledger_draw_reference, pfsp_weights_reference
from tests.test_hip_league import NAMES4, _env, _learner_actions, _near_the_end, _need_gpu
from tests.test_ledger_rules import weighted_draw

pytestmark = pytest.mark.gpu

NAMES = N.CRL_LEDGER_COUNTER_NAMES
TABLE = [3, 1, 2, 5]  # a fixed non-uniform table over NAMES4


class Replay:
    """The books in numpy: feed it every step's (opponent that played, learner reward, done)."""

    def __init__(self, n, agents):
        self.agents = agents
        self.ret, self.len = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.c = {k: np.zeros(agents, np.int64) for k in NAMES}
        self.ignored = 0

    def step(self, played, reward, done):
        assert np.array_equal(reward, np.round(reward))
        self.ret += reward.astype(np.int64)
        self.len += 1
        d = done.astype(bool)
        ok = d & (played >= 0) & (played < self.agents)
        self.ignored += int((d & ~ok).sum())
        a, r = played[ok], self.ret[ok]
        for k, v in (("episodes", 1), ("wins", r > 0), ("losses", r < 0), ("draws", r == 0), ("return_sum", r), ("length_sum", self.len[ok])):
            np.add.at(self.c[k], a, np.asarray(v, np.int64))
        self.ret[d], self.len[d] = 0, 0

    def same_as(self, ledger, rows=None):
        got = ledger.counters()
        for k in NAMES:
            assert np.array_equal(got[k], self.c[k]), (k, got[k], self.c[k])
        assert got["ignored"] == self.ignored
        ret, length, _ = (t.cpu().numpy() for t in ledger.env_state())
        rows = slice(None) if rows is None else rows
        assert np.array_equal(ret[rows], self.ret) and np.array_equal(length[rows], self.len)


def _ledger_run(n, base, steps, acts, table=TABLE, seed=5, league_seed=77):
    """A league over all four agents with a ledger, one uniform draw per env at the start and a WEIGHTED one at every episode end.
    Records of every step: (the assignment before the step, the learner's reward, done, the assignment after it)."""
    lg = LeagueEnvWrapper(_env(n, seed, base), n, NAMES4, seed=league_seed, resample_on_done=True, ledger=True)
    assert lg.ledger.env_id_base == base and lg.ledger.agents == 4
    lg.ledger.set_weights(table)
    lg.reset()
    _near_the_end(lg.env, base)
    lg.reset_opponent()
    rec = []
    for t in range(steps):
        before = lg.assignment
        _, rew, done = lg.step_device(acts[t])
        rec.append((before.cpu().numpy(), rew[:, 0].cpu().numpy().copy(), done.cpu().numpy().astype(bool), lg.assignment.cpu().numpy()))
    out = dict(rec=rec, counters=lg.ledger.counters(), ledger_counts=lg.counts())
    out["ret"], out["len"], out["ctr"] = (x.cpu().numpy() for x in lg.ledger.env_state())
    replay = Replay(n, 4)
    for played, r, d, _ in rec:
        replay.step(played, r, d)
    replay.same_as(lg.ledger)
    out["replay"] = replay
    lg.close()
    return out


_shared = {}


def _whole():
    """1 003 envs x 2 000 steps, run once for the tests below."""
    _need_gpu()
    if "whole" not in _shared:
        n, steps = 1003, 2000
        _shared["acts"] = _learner_actions(steps, n, 13)
        _shared["whole"] = _ledger_run(n, 0, steps, _shared["acts"])
    return _shared["whole"]


def test_books_equal_the_numpy_replay():
    """All six per-agent counters, the per-env running return and length and `ignored` equal the replay of the recorded steps (compared
    inside the run), through several waves of episode ends."""
    run = _whole()
    c, rec = run["counters"], run["rec"]
    ends = sum(int(r[2].sum()) for r in rec)
    waves = sum(bool(r[2].any()) for r in rec)
    print("books: episode ends", ends, "steps with an end", waves, {k: c[k].tolist() for k in NAMES}, "win rate", c["win_rate"].round(3).tolist())
    assert waves >= 3 and c["ignored"] == 0
    assert int(c["episodes"].sum()) == ends and np.array_equal(c["episodes"], c["wins"] + c["losses"] + c["draws"])
    assert (c["episodes"] > 0).all(), "every agent of the pool must have finished episodes"
    assert c["wins"].sum() > 0 and c["losses"].sum() > 0
    assert run["ledger_counts"].sum() == 1003


def test_an_episode_is_booked_to_the_opponent_that_played_it():
    """Envs whose episode ends get their next opponent in the same step: the books must hold the one that played.  Crediting the NEW
    opponent gives other tallies than the device's for this run."""
    run = _whole()
    changed, late = 0, np.zeros(4, np.int64)
    for played, _, d, after in run["rec"]:
        changed += int((d & (after != played)).sum())
        assert np.array_equal(after[~d], played[~d])
        np.add.at(late, after[d], 1)
    assert changed > 100
    assert np.array_equal(run["counters"]["episodes"], run["replay"].c["episodes"]) and not np.array_equal(run["counters"]["episodes"], late)


def test_every_redraw_follows_the_written_rule():
    run = _whole()
    n = 1003
    gid, ctr = np.arange(n), np.zeros(n, np.int64)
    seen = np.zeros(4, np.int64)
    for t, (played, _, d, after) in enumerate(run["rec"]):
        expect = np.where(d, ledger_draw_reference(77, gid, ctr, TABLE), played)
        assert np.array_equal(after, expect), t
        if d.any():
            assert np.array_equal(expect[d], weighted_draw(77, gid[d], ctr[d], TABLE)), t  # the test file's own walk of the table
            np.add.at(seen, after[d], 1)
        ctr += d
    assert np.array_equal(run["ctr"].view(np.uint32), ctr)
    print("redraws per agent", seen.tolist(), "table", TABLE)
    assert seen[3] > seen[0] > seen[1] and seen[2] > seen[1]  # 5 : 3 : 2 : 1 over some thousand draws


def test_shards_draw_and_book_what_the_whole_batch_does():
    whole = _whole()
    acts = _shared["acts"]
    lo = _ledger_run(500, 0, 2000, acts[:, :500])
    hi = _ledger_run(503, 500, 2000, acts[:, 500:])
    for t, (w, a, b) in enumerate(zip(whole["rec"], lo["rec"], hi["rec"])):
        for k, what in enumerate(("assignment before", "reward", "done", "assignment after")):
            assert np.array_equal(w[k], np.concatenate([a[k], b[k]])), (t, what)
    for k in NAMES:
        assert np.array_equal(whole["counters"][k], lo["counters"][k] + hi["counters"][k]), k
    for k in ("ret", "len", "ctr"):
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]])), k


def test_a_zero_weight_agent_loses_its_envs_and_the_host_path_books_too():
    _need_gpu()
    n = 200
    lg = LeagueEnvWrapper(_env(n, 9), n, NAMES4, seed=4, resample_on_done=True, ledger=True)
    lg.ledger.set_weights([1, 0, 2, 1])
    lg.reset()
    st = lg.env.get_state()
    st["num_rounds"] = 20  # every env one round before the end of its episode
    lg.env.set_state(st)
    lg.set_opponents("WEAK")  # the agent of weight 0 holds every env
    assert lg.counts().tolist() == [0, n, 0, 0]
    acts = _learner_actions(3000, n, 2)
    replay, t = Replay(n, 4), 0
    while t < 3000:
        before = lg.assignment.cpu().numpy()
        if t % 2:
            _, rew, done = lg.step_device(acts[t])
            rew, done = rew[:, 0].cpu().numpy().copy(), done.cpu().numpy()
        else:  # the host protocol books as well
            _, rew, done, _ = lg.step(acts[t])
            rew, done = torch.as_tensor(rew).cpu().numpy()[:, 0], torch.as_tensor(done).cpu().numpy()[:, 0]
        replay.step(before, rew, done)
        t += 1
        if t % 25 == 0 and int(lg.ledger.env_state()[2].min()) >= 1:
            break
    assert int(lg.ledger.env_state()[2].min()) >= 1, "not every env was redrawn in 3 000 steps"
    counts = lg.counts()
    print("zero weight: all", n, "envs redrawn after", t, "steps; counts", counts.tolist())
    assert counts[1] == 0 and counts.sum() == n and (counts[[0, 2, 3]] > 0).all()
    replay.same_as(lg.ledger)
    assert replay.c["episodes"][1] >= n  # WEAK played every first episode
    # the pool grows: the ledger follows, the newcomer enters with weight 1 and clean books
    from competitive_rl_amd.policy_serving import BUILTIN_CHECKPOINTS

    lg.add_agent("MINE", BUILTIN_CHECKPOINTS["WEAK"])
    assert lg.ledger.agents == 5 and lg.ledger.weights().tolist() == [1, 0, 2, 1, 1] and lg.ledger.counters()["episodes"][4] == 0
    with pytest.raises(N.CrlError, match="sum"):
        lg.ledger.set_weights([0, 0, 0, 0, 0])
    with pytest.raises(N.CrlError, match="sum"):
        lg.ledger.set_weights([0xFFFFFFFF, 1, 0, 0, 0])
    with pytest.raises(N.CrlError, match="floor"):
        lg.ledger.pfsp_weights(floor=1 << 30)
    assert lg.ledger.weights().tolist() == [1, 0, 2, 1, 1]
    # seed() re-keys the ledger with the league: the next redraws are draw 0 under the new key
    lg.seed(12)
    assert not lg.ledger.env_state()[2].any()
    ids = lg.ledger.update(lg.assignment, torch.zeros((n, 2), device=lg.device), torch.ones((n,), dtype=torch.uint8, device=lg.device), redraw=True)
    assert np.array_equal(ids.cpu().numpy(), ledger_draw_reference(12, np.arange(n), 0, [1, 0, 2, 1, 1]))
    led = lg.ledger
    lg.close()
    assert led._h is None  # a ledger the wrapper built is closed with it


def _synthetic(n, agents, steps, seed, lo=-1, hi=None):
    """Made-up steps on the device: ids in [lo, hi) (some outside the pool), rewards in {-1, 0, 1}, one done flag in eight."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    hi = agents + 1 if hi is None else hi
    assign = torch.randint(lo, hi, (steps, n), generator=g, device="cuda", dtype=torch.int32)
    reward = torch.zeros((steps, n, 2), device="cuda")
    reward[:, :, 0] = torch.randint(-1, 2, (steps, n), generator=g, device="cuda").float()
    reward[:, :, 1] = 7.0  # the opponent's column must never be read
    done = (torch.randint(0, 8, (steps, n), generator=g, device="cuda") == 0).to(torch.uint8)
    return assign, reward, done


@pytest.mark.parametrize("n, agents", [pytest.param(n, 5, id=str(n)) for n in (1, 63, 64, 65, 257, 1003)]
                         + [pytest.param(n, 16, id=f"{n}-full-pool") for n in (65, 257)])
def test_made_up_steps_with_losses_draws_and_ids_outside_the_pool(n, agents):
    """What Pong cannot show: drawn episodes (return 0), ids outside the pool (-> `ignored`), the reward's column stride; at sizes
    around the wavefront and the block.  Every second step asks for redraws and takes the ids in place.  At step 20 EVERY env is done
    and env i holds id (i mod (agents + 2)) - 1: a wavefront then carries every key of the pool plus -1 and `agents`, the last one the
    lanes beyond n as well -- with the full pool of 16 the most rounds the step's grouping loop can run."""
    _need_gpu()
    steps = 60
    led = LeagueLedger(n, agents, "cuda:0", seed=31, env_id_base=(1 << 33) + 5)
    table = [2, 0, 1, 4, 1] if agents == 5 else [(3 * k) % 5 for k in range(agents)]
    led.set_weights(table)
    assign, reward, done = _synthetic(n, agents, steps, n)
    done[20] = 1
    assign[20] = torch.arange(n, device="cuda", dtype=torch.int32) % (agents + 2) - 1
    replay, ctr, gid = Replay(n, agents), np.zeros(n, np.int64), (1 << 33) + 5 + np.arange(n)
    for t in range(steps):
        a, r, d = assign[t].cpu().numpy(), reward[t, :, 0].cpu().numpy(), done[t].cpu().numpy().astype(bool)
        redraw = t % 2 == 1
        ids = led.update(assign[t], reward[t] if t % 3 else reward[t, :, 0].contiguous(), done[t], redraw=redraw, out=assign[t] if redraw else None)
        expect = np.where(d, ledger_draw_reference(31, gid, ctr, table), a) if redraw else a
        ctr += d & redraw
        assert np.array_equal(ids.cpu().numpy(), expect), t
        replay.step(a, r, d)
    replay.same_as(led)
    c = led.counters()
    if n >= 63:
        assert c["ignored"] > 0 and c["draws"].sum() > 0 and c["losses"].sum() > 0 and (c["return_sum"] != 0).any()
    assert np.array_equal(led.env_state()[2].cpu().numpy().view(np.uint32), ctr)
    led.reset()
    c = led.counters()
    assert all(not c[k].any() for k in NAMES) and c["ignored"] == 0 and not led.env_state()[0].any() and not led.env_state()[1].any()
    assert np.array_equal(led.env_state()[2].cpu().numpy().view(np.uint32), ctr) and led.weights().tolist() == table  # reset keeps these
    led.seed(32)
    assert not led.env_state()[2].any()
    ids = led.update(assign[0], reward[0], torch.ones_like(done[0]), redraw=True)
    assert np.array_equal(ids.cpu().numpy(), ledger_draw_reference(32, gid, 0, table))
    led.close()


def _random_books(rs):
    c = np.zeros((N.CRL_LEDGER_COUNTERS, N.CRL_LEAGUE_MAX_AGENTS), np.int64)
    e = rs.randint(0, 10 ** rs.randint(1, 13, 16), dtype=np.int64)
    e[:3] = [0, 1, 10 ** 6]
    wins = (e * rs.random_sample(16)).astype(np.int64)
    wins[2], wins[3], wins[4] = e[2], e[3], 0  # always beaten / never beaten
    draws = ((e - wins) * rs.random_sample(16)).astype(np.int64)
    c[0], c[1], c[3], c[2] = e, wins, draws, e - wins - draws
    c[4], c[5] = rs.randint(-10 ** 9, 10 ** 9, 16), e * 700
    return c


def test_pfsp_weights_on_the_device_equal_the_numpy_rule_bit_for_bit():
    _need_gpu()
    rs = np.random.RandomState(3)
    for agents in (16, 5, 1):
        led = LeagueLedger(70, agents, "cuda:0")
        for trial in range(6):
            own, passed = _random_books(rs), _random_books(rs)
            sd = led.state_dict()
            sd["counters"] = own
            led.load_state_dict(sd)
            assert np.array_equal(led.counters_device().cpu().numpy(), own)
            t = torch.from_numpy(passed).cuda()
            for mode, k, floor in (("hard", 1, 1), ("hard", 2, 1), ("hard", 3, 0), ("variance", 2, 1), ("variance", 1, 0), ("hard", 2, 1000)):
                led.pfsp_weights(mode, k, floor)
                assert np.array_equal(led.weights_device().cpu().numpy(), pfsp_weights_reference(own, agents, mode, k, floor).astype(np.int64)), (mode, k, floor)
                led.pfsp_weights(mode, k, floor, counters=t)
                assert np.array_equal(led.weights_device().cpu().numpy(), pfsp_weights_reference(passed, agents, mode, k, floor).astype(np.int64)), (mode, k, floor)
        led.close()


def test_a_fresh_ledger_continues_from_a_state_dict():
    _need_gpu()
    n, agents, steps = 777, 4, 40
    assign, reward, done = _synthetic(n, agents, 2 * steps, 8, lo=0, hi=agents)
    a = LeagueLedger(n, agents, "cuda:0", seed=6, env_id_base=1000)
    a.set_weights([1, 7, 0, 2])
    for t in range(steps):
        a.update(assign[t], reward[t], done[t], redraw=True)
    a.pfsp_weights("hard", 2, 1)
    sd = a.state_dict()
    b = LeagueLedger(n, agents, "cuda:0", seed=999, env_id_base=1000)
    b.load_state_dict(sd)
    for t in range(steps, 2 * steps):
        assert torch.equal(a.update(assign[t], reward[t], done[t], redraw=True), b.update(assign[t], reward[t], done[t], redraw=True)), t
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb) and sa["draw_ctr"].any() and sa["counters"][0].sum() > steps
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.close(), b.close()


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_a_refused_load_leaves_the_ledger_as_it_was():
    """An all-zero weight table and counters of the wrong size are refused BEFORE anything is written (the library would refuse the
    table only after the counters and the per-env state had been replaced)."""
    _need_gpu()
    n, agents, steps = 65, 3, 12
    assign, reward, done = _synthetic(n, agents, steps, 4)
    led = LeagueLedger(n, agents, "cuda:0", seed=9, env_id_base=40)
    led.set_weights([4, 0, 3])
    for t in range(steps):
        led.update(assign[t], reward[t], done[t], redraw=True)
    before = led.state_dict()
    assert before["counters"][0].sum() > 0 and before["draw_ctr"].any() and before["ret"].any()
    other = {"agents": agents, "seed": 1234, "counters": before["counters"] + 5, "ignored": before["ignored"] + 1, "ret": before["ret"] + 1,
             "len": before["len"] + 1, "draw_ctr": before["draw_ctr"] + np.uint32(1), "weights": np.array([1, 2, 3], np.uint32)}
    for bad in (dict(other, weights=np.zeros(agents, np.uint32)), dict(other, counters=np.zeros((N.CRL_LEDGER_COUNTERS, 15), np.int64))):
        with pytest.raises(ValueError, match="load_state_dict"):
            led.load_state_dict(bad)
        _same_state(led.state_dict(), before)
    led.load_state_dict(other)  # (what was refused differs from a good one in that entry alone)
    _same_state(led.state_dict(), other)
    led.close()


def test_a_duplicate_name_is_refused_and_the_pool_stays():
    _need_gpu()
    from competitive_rl_amd.policy_serving import BUILTIN_CHECKPOINTS

    lg = LeagueEnvWrapper(_env(1, 3), 1, NAMES4, ledger=True)
    lg.add_agent("MINE", BUILTIN_CHECKPOINTS["WEAK"])
    names, kinds, styles, weights = list(lg.agent_names), list(lg._kinds), lg.sampling(), lg.ledger.weights()
    for name in ("MINE", "RANDOM"):
        with pytest.raises(ValueError, match="is in the pool already"):
            lg.add_agent(name, BUILTIN_CHECKPOINTS["MEDIUM"], temperature=1.0)
    assert lg.agent_names == names and lg._kinds == kinds and lg.sampling() == styles and lg.counts().tolist() == [0, 0, 0, 1, 0]
    assert lg.ledger.agents == 5 and np.array_equal(lg.ledger.weights(), weights) and weights.tolist() == [1] * 5
    lg.close()


def test_step_device_with_a_ledger_does_no_host_work():
    """The method of tests/test_hip_league.py::test_step_device_does_no_host_work with the ledger in the loop: 50 steps with books, weighted
    redraws and a pfsp_weights() call every 10 steps, enqueued behind a long-running launch, leave the host before that launch ends."""
    _need_gpu()
    n = 4096
    lg = LeagueEnvWrapper(_env(n, 3), n, NAMES4, seed=1, resample_on_done=True, ledger=True)
    lg.reset()
    _near_the_end(lg.env)
    lg.reset_opponent()
    acts = _learner_actions(60, n, 16)
    for t in range(10):  # warm-up: lazy allocations, kernel loading
        lg.step_device(acts[t])
    lg.ledger.pfsp_weights()
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
        if t % 10 == 0:
            lg.ledger.pfsp_weights("hard", 2, 1)
    host = time.perf_counter() - t0
    still_busy = not busy.query()
    torch.cuda.synchronize()
    print("50 step_device calls with a ledger took the host", round(host * 1e3, 2), "ms behind", reps, "queued matrix products; device still busy:", still_busy)
    assert still_busy, "the host waited for the device inside step_device"
    assert prev[0].shape == (n, 2, 1, 42, 42) and lg.ledger.counters()["episodes"].sum() > 0
    lg.close()


def test_books_at_65536_envs_on_512_sampled_envs():
    _need_gpu()
    n, steps = 65536, 150
    lg = LeagueEnvWrapper(_env(n, 6), n, NAMES4, seed=2, resample_on_done=True, ledger=True)
    lg.ledger.set_weights(TABLE)
    lg.reset()
    _near_the_end(lg.env)
    lg.reset_opponent()
    rows = torch.as_tensor(np.sort(np.random.RandomState(6).choice(n, 512, replace=False)), device=lg.device)
    acts = _learner_actions(steps, n, 17)
    ends = torch.zeros((), dtype=torch.int64, device=lg.device)
    rec = []
    for t in range(steps):
        before = lg.assignment[rows]
        _, rew, done = lg.step_device(acts[t])
        ends += done.sum()
        rec.append((before, rew[rows, 0].clone(), done[rows].clone()))
    replay = Replay(512, 4)
    for before, r, d in rec:
        replay.step(before.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy())
    c = lg.ledger.counters()
    print("65 536 envs: episode ends", int(ends), "per agent", c["episodes"].tolist(), "of the sample", replay.c["episodes"].tolist())
    assert int(ends) > 0 and replay.c["episodes"].sum() > 0 and int(c["episodes"].sum()) == int(ends) and c["ignored"] == 0
    assert np.array_equal(c["episodes"], c["wins"] + c["losses"] + c["draws"]) and (replay.c["episodes"] <= c["episodes"]).all()
    ret, length, _ = (x[rows].cpu().numpy() for x in lg.ledger.env_state())
    assert np.array_equal(ret, replay.ret) and np.array_equal(length, replay.len)
    assert lg.counts().sum() == n
    lg.close()


def test_a_league_without_a_ledger_is_the_league_of_before():
    """`ledger=None` adds nothing: two identically seeded leagues, one built with the keyword and one without, show the same
    assignment, counts and outputs over a short run with uniform redraws (crl_league_resample's), and own no ledger."""
    _need_gpu()
    n, steps = 520, 300
    a = LeagueEnvWrapper(_env(n, 2), n, NAMES4, seed=3, resample_on_done=True)
    b = LeagueEnvWrapper(_env(n, 2), n, NAMES4, seed=3, resample_on_done=True, ledger=None)
    assert a.ledger is None and b.ledger is None
    a.reset(), b.reset()
    _near_the_end(a.env), _near_the_end(b.env)
    a.reset_opponent(), b.reset_opponent()
    acts = _learner_actions(steps, n, 18)
    from tests.test_league_rules import DOMAIN_OPPONENT, league_draw

    expect, ctr, ends = league_draw(3, np.arange(n), 0, DOMAIN_OPPONENT, 4), np.ones(n, np.int64), 0
    for t in range(steps):
        (ba, ra, da), (bb, rb, db) = a.step_device(acts[t]), b.step_device(acts[t])
        assert torch.equal(ba, bb) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(a._act, b._act), t
        d = da.cpu().numpy().astype(bool)
        expect = np.where(d, league_draw(3, np.arange(n), ctr, DOMAIN_OPPONENT, 4), expect)  # the UNIFORM rule, the league's own domain word
        ctr += d
        ends += int(d.sum())
        assert np.array_equal(a.assignment.cpu().numpy(), expect) and torch.equal(a.assignment, b.assignment), t
    assert ends > 0 and np.array_equal(a.counts(), b.counts()) and np.array_equal(a.counts(), np.bincount(expect, minlength=4))
    a.close(), b.close()

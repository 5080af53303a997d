"""Full-size ActorCritic agents served per env (LeagueEnvWrapper.add_full_agent / LeagueArena.add_full_agent, crl_pool_add_full, the
list form of csrc/pong_policy_full.hip) on the device.  The list launch must compute, for every env of the agent, exactly what the
dense launch of a ``Policy(use_light_model=False)`` computes on the same frames: tolerance 0 wherever a dense policy is the
reference; the float64 test takes the budget of tests/policy_f64_cases.py (a rule over references only)."""
import functools

import numpy as np
import pytest
import torch

from competitive_rl_amd.league import LeagueEnvWrapper, league_sample_reference
from tests import policy_f64_cases as C
from tests.policy_f64_child import full_policy, light_policy
from tests.policy_full_weights import make_weights
from tests.test_hip_league import _env, _learner_actions, _near_the_end
from tests.test_hip_league_sampling import MARGIN

pytestmark = pytest.mark.gpu

CALLS = 8
RULE, WEAK, BIG_A, BIG_B = 0, 1, 2, 3  # pool order of _league


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _frames(n, calls=CALLS):
    """uint8 [calls, n, 1, 42, 42] on the device, seeded; read-only by convention"""
    g = torch.Generator(device="cuda").manual_seed(1000 + n)
    return torch.randint(0, 256, (calls, n, 1, 42, 42), generator=g, device="cuda", dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _reference(n, calls=CALLS):
    """{agent id: (logits [calls, n, 3], actions [calls, n])} of dense policies of n envs fed _frames(n): computed once per size.  The
    league pushes every env's frame on every call, so an env's history is the dense policy's whatever the assignment was."""
    out = {}
    for a, pol in ((BIG_A, full_policy(make_weights(5), n)), (BIG_B, full_policy(make_weights(3), n)), (WEAK, light_policy(C.shipped("weak"), n))):
        lg, act = [], []
        for t in range(calls):
            act.append(pol.act_device(_frames(n, calls)[t], want_logits=True).clone())
            lg.append(pol.logits().clone())
        out[a] = (torch.stack(lg), torch.stack(act))
        pol.close()
    return out


def _league(n, scratch_rows=None, seed=5, base=0, big_b=True):
    lg = LeagueEnvWrapper(_env(n, 21, base), n, ["RULE_BASED", "WEAK"], seed=seed)
    lg.add_full_agent("BIG_A", make_weights(5), scratch_rows=scratch_rows)
    if big_b:
        lg.add_full_agent("BIG_B", make_weights(3))
    lg.record_logits = True
    return lg


def _assignment(n, k, seed, mixed=False):
    """BIG_A holds k envs scattered over the batch; BIG_B, WEAK and RULE_BASED share the rest, interleaved (no list is a run of envs):
    env i on the (i mod 3)-th of them, or with `mixed` on a seeded random one"""
    rs = np.random.RandomState(seed)
    a = np.array([BIG_B, WEAK, RULE])[rs.randint(0, 3, n) if mixed else np.arange(n) % 3]
    a[rs.permutation(n)[:k]] = BIG_A
    return a


def _act(lg, frame):
    lg.prev_opponent_obs = frame
    return lg._fill_actions(torch.zeros((lg.num_envs,), dtype=torch.int32, device=lg.device))[:, 1].clone()


def _check_call(lg, t, assign, act, ref, who=(WEAK, BIG_A, BIG_B)):
    for a in who:
        rows = torch.from_numpy(np.flatnonzero(assign == a)).to(lg.device)
        assert torch.equal(lg.logits()[rows], ref[a][0][t][rows]), (t, lg.agent_names[a])
        assert torch.equal(act[rows], ref[a][1][t][rows]), (t, lg.agent_names[a])
    assert bool((act[torch.from_numpy(assign == RULE).to(lg.device)] == 999).all())


@pytest.mark.parametrize("k", [0, 1, 7, 128, 129, "switch"])
def test_list_launch_equals_the_dense_launch_bit_for_bit(k):
    """BIG_A on 0, 1, 7, 128 and 129 of 261 envs (the empty list, a lone row, no multiple of 8, both sides of conv3's 128-row tile) beside
    a second full-size agent, WEAK and RULE_BASED; "switch": 129 envs, then after call 4 another 7 and a reshuffled rest, so envs change hands between all
    four agents, in every direction, while the shared ring keeps their history."""
    _need_gpu()
    n = 261
    ref = _reference(n)
    lg = _league(n)
    assert lg.agent_names == ["RULE_BASED", "WEAK", "BIG_A", "BIG_B"]
    plan = [_assignment(n, 129, 1)] * 4 + [_assignment(n, 7, 2, mixed=True)] * 4 if k == "switch" else [_assignment(n, k, 3)] * CALLS
    for t in range(CALLS):
        if t == 0 or plan[t] is not plan[t - 1]:
            lg.set_opponents(plan[t])
            lists = lg.agent_lists()
            assert sorted(lists) == ["BIG_A", "BIG_B", "WEAK"]
            for a in (WEAK, BIG_A, BIG_B):
                assert np.array_equal(lists[lg.agent_names[a]], np.flatnonzero(plan[t] == a))
        _check_call(lg, t, plan[t], _act(lg, _frames(n)[t]), ref)
    if k == "switch":
        moves = {(int(a), int(b)) for a, b in zip(plan[0], plan[-1]) if a != b}
        assert (plan[0] != plan[-1]).sum() > 100 and len(moves) == 12, moves  # every agent hands envs to every other one
        with pytest.raises(ValueError, match="add_agent"):
            lg.add_full_agent("L", C.shipped("weak"))
        with pytest.raises(ValueError, match="add_agent"):
            lg.add_full_agent("L", light_policy(C.shipped("weak"), 2))
        with pytest.raises(ValueError, match="full-size ActorCritic is not"):
            lg.add_agent("F", make_weights(5))
        with pytest.raises(ValueError, match="42x42"):
            import competitive_rl_amd as crl

            big = LeagueEnvWrapper(crl.make_envs("cPongDouble-v0", num_envs=2, log_dir=None, resized_dim=84, frame_stack=None), 2, ["RULE_BASED"])
            big.add_full_agent("BIG", make_weights(5))
        assert lg.agent_names == ["RULE_BASED", "WEAK", "BIG_A", "BIG_B"]
    lg.close()


F64_POOL = {"dense": (("FULL", "full"), ("SELECTOR", "full_selector"), ("WIDE", "full_wide")), "sparse": (("FULL", "full"),)}


@pytest.mark.parametrize("kind", sorted(F64_POOL))
def test_list_launch_against_float64(kind):
    """The full-size weight sets that have a batch of this input kind in one pool next to RULE_BASED, 131 envs (one conv3 tile plus
    3 rows over all lists); every row against the float64 logits of the weight set that serves it."""
    _need_gpu()
    n = 131
    lg = LeagueEnvWrapper(_env(n, 21), n, ["RULE_BASED"], seed=5)
    for a, ws in F64_POOL[kind]:
        lg.add_full_agent(a, C.weight_set(ws)[0])
    lg.record_logits = True
    assign = np.arange(len(F64_POOL[kind]) + 1)[(np.arange(n) + 1) % (len(F64_POOL[kind]) + 1)]
    lg.set_opponents(assign)
    frames = C.case("full", kind).frames_for(n)  # (the frames of a kind do not depend on the weight set)
    logits, acts = [], []
    for t in range(C.CALLS):
        a = _act(lg, torch.from_numpy(frames[t][:, None]).to(lg.device)).cpu().numpy()
        if t >= C.WARMUP:
            logits.append(lg.logits().cpu().numpy().copy()), acts.append(a)
    assert (acts[-1][assign == 0] == 999).all()
    for a, ws in F64_POOL[kind]:
        rows = np.flatnonzero(assign == lg.agent_names.index(a))
        assert len(rows) > 8
        C.judge("league full-size list launch (%s)" % a, C.case(ws, kind), np.stack(logits), np.stack(acts), n, rows=rows)
    lg.close()


@pytest.mark.parametrize("scratch_rows", [48, 100])
def test_passes_over_a_small_scratch(scratch_rows):
    """100 of 130 envs on BIG_A with a scratch of 48 rows (three passes, the last one ragged: 48 + 48 + 4) and of 100 rows (the pass
    boundary falls on the count; the second pass is empty); BIG_B shares the scratch."""
    _need_gpu()
    n = 130
    ref = _reference(n)
    lg = _league(n, scratch_rows=scratch_rows, big_b=False)
    with pytest.raises(Exception, match="scratch_rows"):
        lg.add_full_agent("BIG_B", make_weights(3), scratch_rows=64)
    assert lg.agent_names == ["RULE_BASED", "WEAK", "BIG_A"]
    lg.add_full_agent("BIG_B", make_weights(3), scratch_rows=scratch_rows)
    assign = _assignment(n, 100, 4)
    lg.set_opponents(assign)
    assert lg.counts().tolist() == [int((assign == a).sum()) for a in range(4)] and lg.counts()[BIG_A] == 100
    for t in range(CALLS):
        _check_call(lg, t, assign, _act(lg, _frames(n)[t]), ref)
    lg.close()


def test_sampled_and_explored_actions_are_drawn_with_the_envs_id():
    """BIG_A at temperature 1, epsilon 0.1 on a scattered list of a league whose ids start at 1000: the draw of env i is keyed by
    1000 + i (a row-position id would give other actions: the list is not in env order); BIG_B stays greedy."""
    _need_gpu()
    n, calls, seed, base = 70, 12, 77, 1000
    assign = _assignment(n, 30, 5)
    frames = _frames(n, calls)
    runs = {}
    for sampled in (False, True):
        lg = _league(n, seed=seed, base=base)
        if sampled:
            lg.set_sampling("BIG_A", 1.0, 0.1)
            assert lg.sampling()["BIG_A"] == (1.0, pytest.approx(0.1)) and lg.sampling()["BIG_B"] == (0.0, 0.0)
        lg.set_opponents(assign)
        acts, logits = [], []
        for t in range(calls):
            acts.append(_act(lg, frames[t]).cpu().numpy()), logits.append(lg.logits().cpu().numpy().copy())
        runs[sampled] = (np.stack(acts), np.stack(logits))
        lg.close()
    (act0, lg0), (act1, lg1) = runs[False], runs[True]
    assert np.array_equal(lg0, lg1)  # the logits are the raw ones whatever the style
    rows = np.flatnonzero(assign == BIG_A)
    steps = np.arange(calls)[:, None]
    want, explored, margin = league_sample_reference(seed, (base + rows)[None, :], steps, lg1[:, rows], 1.0, 0.1)
    close = ~explored & (margin < MARGIN)  # tests/test_hip_league_sampling.py's rule: float32 expf may decide such a draw the other way
    print("sampled draws", int((~explored).sum()), "explored", int(explored.sum()), "left out (margin < 1e-5)", int(close.sum()))
    assert close.sum() <= 1e-3 * (~explored).sum() and explored.any() and np.array_equal(act1[:, rows][~close], want[~close])
    by_row = league_sample_reference(seed, (base + np.arange(len(rows)))[None, :], steps, lg1[:, rows], 1.0, 0.1)[0]
    assert (by_row != want).any() and (act1[:, rows] != act0[:, rows]).any()
    others = np.flatnonzero(assign != BIG_A)
    assert np.array_equal(act1[:, others], act0[:, others])


def test_arena_serves_a_full_size_agent_in_both_seats():
    _need_gpu()
    from competitive_rl_amd.arena import LeagueArena

    n, calls = 66, 6
    arena = LeagueArena(_env(n, 4), n, ["RULE_BASED", "MEDIUM"], seed=11)
    arena.add_full_agent("BIG", make_weights(5))
    arena.record_logits = True
    assert arena.agent_names == ["RULE_BASED", "MEDIUM", "BIG"] and arena.counters()["episodes"].shape == (3, 3)
    assert arena.weights().tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    seat_agent = ((np.arange(2 * n) * 2 + np.arange(2 * n) // 5) % 3).reshape(n, 2)
    arena.set_pairs(seat_agent[:, 0], seat_agent[:, 1])
    big = np.flatnonzero(seat_agent.reshape(-1) == 2)
    assert (big % 2 == 0).sum() > 8 and (big % 2 == 1).sum() > 8  # both seats
    rows = torch.from_numpy(big).to(arena.device)
    pol = full_policy(make_weights(5), 2 * n)
    frames = _frames(2 * n, calls)
    for t in range(calls):
        arena._buf = frames[t].reshape(n, 2, 1, 42, 42)
        a = arena._fill_actions().reshape(-1).clone()
        b = pol.act_device(frames[t], want_logits=True)
        assert torch.equal(arena.logits()[rows], pol.logits()[rows]) and torch.equal(a[rows], b[rows]), t
    assert sorted(arena.state_dict()["agent_names"]) == ["BIG", "MEDIUM", "RULE_BASED"]
    with pytest.raises(ValueError, match="add_agent"):
        arena.add_full_agent("L", C.shipped("weak"))
    pol.close(), arena.close()


def test_draws_with_a_full_size_agent_in_the_pool():
    """resample_on_done with a ledger: the lists follow the redraws step by step, BIG plays whole episodes and they are booked to it."""
    _need_gpu()
    n, steps = 64, 200
    lg = LeagueEnvWrapper(_env(n, 9), n, ["RANDOM", "WEAK", "RULE_BASED"], seed=13, resample_on_done=True, ledger=True)
    lg.add_full_agent("BIG", make_weights(5))
    assert lg.ledger.agents == 4
    lg.reset()
    _near_the_end(lg.env)
    lg.reset_opponent()  # one draw per env over the four agents
    acts = _learner_actions(steps, n, 3)
    seen = set()
    for t in range(steps):
        lg.step_device(acts[t])
        assign = lg.assignment.cpu().numpy()
        assert lg.counts().sum() == n and np.array_equal(lg.counts(), np.bincount(assign, minlength=4))
        lists = lg.agent_lists()
        assert sorted(lists) == ["BIG", "WEAK"]
        assert np.array_equal(lists["WEAK"], np.flatnonzero(assign == 1)) and np.array_equal(lists["BIG"], np.flatnonzero(assign == 3))
        seen.add(len(lists["BIG"]))
    books = lg.ledger.counters()
    assert len(books["episodes"]) == 4 and books["ignored"] == 0
    print("episodes per agent", books["episodes"], "sizes of BIG's list", sorted(seen))
    assert books["episodes"][3] >= 1 and len(seen) > 1
    lg.close()


def test_an_idle_full_size_agent_changes_nothing():
    _need_gpu()
    n, calls = 65, 6
    assign = np.arange(n) % 3
    out = []
    for idle in (False, True):
        lg = LeagueEnvWrapper(_env(n, 21), n, ["RULE_BASED", "WEAK", "MEDIUM"], seed=5)
        if idle:
            lg.add_full_agent("BIG", make_weights(5))
        lg.record_logits = True
        lg.set_opponents(assign)
        got = []
        for t in range(calls):
            got.append((_act(lg, _frames(n, calls)[t]), lg.logits().clone()))
        if idle:
            assert lg.counts().tolist() == [22, 22, 21, 0] and len(lg.agent_lists()["BIG"]) == 0
        out.append(got)
        lg.close()
    for (a0, l0), (a1, l1) in zip(*out):
        assert torch.equal(a0, a1) and torch.equal(l0, l1)

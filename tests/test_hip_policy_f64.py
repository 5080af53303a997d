"""The CNN opponents' logits on the device against a float64 forward pass (oracle/policy_oracle.forward64), on every path that
computes logits: crl_policy_act of the light networks (act_device, compute_action), the league's list launch and the arena, the
full-size network's three kernels, and the superseded packed-FMA and fp32-MFMA kernels of the profiling library.

Tolerance: the budget of tests/policy_f64_cases.py -- FACTOR x the worst error of the float32 references (BLAS order, sequential
order) against float64 on the same batch, never below two float32 ulps of the largest |logit|; computed from references only.
tests/test_policy_f64_reference.py shows on the CPU that a kernel which loses conv1's third bf16 term, or feeds conv2 / conv3
16-bit operands, misses this budget by a factor of at least two on the batches used here.  Actions equal the float64 argmax wherever
the float64 top-two gap exceeds 2 x budget.  Ties (actor_w = 0) and single-pixel impulses have tolerance 0 resp. the budget of their
own two-row batch.  Every comparison prints its measured line under -s (docs/LAB_NOTES_policy_numerics.md has the table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import policy_f64_cases as C  # noqa: E402
from tests.policy_f64_child import (CHILD_SIZES, TIE_ENVS, abl_library, full_policy, light_policy, run_calls, run_impulses,  # noqa: E402
                                    run_ties)

LIGHT = sorted(C.LIGHT_CASES)
FULL = sorted(C.FULL_CASES)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


# ---- logits and actions against float64
@pytest.mark.parametrize("n", [11, 2059])
@pytest.mark.parametrize("ws,kind", LIGHT)
def test_light_act_device(ws, kind, n):
    """11 = a group of 8 plus 3; 2 059 = 8 x 257 + 3: more groups than the 256 persistent workgroups, so groups are handed on by the
    ticket counter and the pipelined epilogue (finish_group of the previous group beside the next one's tiles) runs."""
    _need_gpu()
    c = C.case(ws, kind)
    pol = light_policy(c.weights, n)
    lg, act = run_calls(pol, c.frames_for(n))
    pol.close()
    C.judge("light act_device", c, lg, act, n)


@pytest.mark.parametrize("ws,kind", LIGHT)
def test_light_compute_action_on_a_stack(ws, kind):
    """Policy.compute_action(stack): the same stacks handed over whole, between calls that advance the policy's own history."""
    _need_gpu()
    n = 11
    c = C.case(ws, kind)
    stacks = C.stacks_of(c.frames_for(n))[C.WARMUP:]
    pol = light_policy(c.weights, n)
    lg, act = [], []
    for t in range(len(stacks)):
        pol.act_device(torch.from_numpy(c.frames_for(n)[t][:, None]).cuda())  # (moves the ring head on)
        act.append(pol.compute_action(stacks[t], deterministic=True).reshape(-1).cpu().numpy())
        lg.append(pol.logits().cpu().numpy().copy())
    pol.close()
    C.judge("light compute_action", c, np.stack(lg), np.stack(act), n)


LEAGUE_POOL = (("WEAK", "weak"), ("MEDIUM", "medium"), ("SELECTOR", "light_selector"), ("WIDE", "light_wide"))


def _league_agents(kind):
    """(agent name, weight set) of the pool's CNN agents that have a batch of this input kind"""
    return [(a, ws) for a, ws in LEAGUE_POOL if (ws, kind) in C.LIGHT_CASES]


def _add_own_agents(lg):
    for a, ws in LEAGUE_POOL[2:]:
        lg.add_agent(a, C.weight_set(ws)[0])


@pytest.mark.parametrize("n", [9, 65])
@pytest.mark.parametrize("kind", ["ones", "dense", "sparse", "bright"])
def test_league_list_launch(kind, n):
    """crl_league_act: one list launch per CNN agent over a ragged assignment (the group-edge sizes of tests/test_hip_league.py); every
    row against the float64 logits of the weight set that serves it.  RULE_BASED rows in between keep the lists apart."""
    _need_gpu()
    from competitive_rl_amd.league import LeagueEnvWrapper
    from tests.test_hip_league import _env

    lg = LeagueEnvWrapper(_env(n, 21), n, ["RULE_BASED", "WEAK", "MEDIUM"], seed=5)
    _add_own_agents(lg)
    lg.record_logits = True
    agents = _league_agents(kind)
    ids = [0] + [lg.agent_names.index(a) for a, _ in agents]
    assign = np.array(ids)[(np.arange(n) + 1) % len(ids)]
    lg.set_opponents(assign)
    frames = C.case(agents[0][1], kind).frames_for(n)  # (the frames of a kind do not depend on the weight set)
    mine = torch.zeros((n,), dtype=torch.int32, device=lg.device)
    logits, acts = [], []
    for t in range(C.CALLS):
        lg.prev_opponent_obs = torch.from_numpy(frames[t][:, None]).to(lg.device)
        a = lg._fill_actions(mine)[:, 1].cpu().numpy().copy()
        if t >= C.WARMUP:
            logits.append(lg.logits().cpu().numpy().copy()), acts.append(a)
    assert (acts[-1][assign == 0] == 999).all()
    for a, ws in agents:
        rows = np.flatnonzero(assign == lg.agent_names.index(a))
        assert len(rows) > 0
        C.judge("league list launch (%s)" % a, C.case(ws, kind), np.stack(logits), np.stack(acts), n, rows=rows)
    lg.close()


@pytest.mark.parametrize("kind", ["ones", "dense", "sparse"])
def test_arena_both_seats(kind):
    """LeagueArena at 130 envs (tests/test_hip_arena.py's size: 260 seats, no list a multiple of 8): the seats' frames are made up, the
    pairs fixed; row 2 i + seat of logits() against the float64 logits of the agent in that seat."""
    _need_gpu()
    from competitive_rl_amd.arena import LeagueArena
    from tests.test_hip_league import _env

    n = 130
    arena = LeagueArena(_env(n, 4), n, ["RULE_BASED", "WEAK", "MEDIUM"], seed=11)
    _add_own_agents(arena)
    arena.record_logits = True
    agents = _league_agents(kind)
    ids = np.array([0] + [arena.agent_names.index(a) for a, _ in agents])
    seat_agent = ids[(np.arange(2 * n) * 3 + np.arange(2 * n) // 7) % len(ids)].reshape(n, 2)
    arena.set_pairs(seat_agent[:, 0], seat_agent[:, 1])
    frames = C.case(agents[0][1], kind).frames_for(2 * n)
    logits, acts = [], []
    for t in range(C.CALLS):
        arena._buf = torch.from_numpy(frames[t].reshape(n, 2, 1, 42, 42)).to(arena.device)
        a = arena._fill_actions().cpu().numpy().reshape(-1).copy()
        if t >= C.WARMUP:
            logits.append(arena.logits().cpu().numpy().copy()), acts.append(a)
    for a, ws in agents:
        rows = np.flatnonzero(seat_agent.reshape(-1) == arena.agent_names.index(a))
        assert len(rows) > 8
        C.judge("arena (%s)" % a, C.case(ws, kind), np.stack(logits), np.stack(acts), 2 * n, rows=rows)
    arena.close()


@pytest.mark.parametrize("n", [3, 130])
@pytest.mark.parametrize("ws,kind", FULL)
def test_full_size(ws, kind, n):
    """3 envs; 130 = one conv3 tile of 128 envs plus 2 (conv2's ragged eighth tile of 16 positions is in every env)."""
    _need_gpu()
    c = C.case(ws, kind)
    pol = full_policy(c.weights, n)
    lg, act = run_calls(pol, c.frames_for(n))
    pol.close()
    C.judge("full-size", c, lg, act, n)


# ---- exact cases
def _judge_ties(tag, logits, actions):
    """logits [4 biases, calls, n, 3]: equal to actor_b (tolerance 0; -0.0 + 0.0 = +0.0 is the float64 forward's answer as well), and
    the first index of the maximum plays"""
    for i, (bias, want) in enumerate(zip(C.TIE_BIASES, C.TIE_ACTIONS)):
        assert np.array_equal(logits[i], np.broadcast_to(np.array(bias, np.float32), logits[i].shape)), (tag, bias)
        assert (actions[i] == want).all(), (tag, bias, np.unique(actions[i]))


def _judge_impulses(tag, wts, full, logits):
    """logits [4 head positions, 25, 3]: logits(impulse) - logits(zero) against the float64 difference, within the budget of the
    two-row batch (impulse, zero)"""
    want, budgets = C.impulse_reference(wts, full)
    got = logits[:, :-1].astype(np.float64) - logits[:, -1:].astype(np.float64)
    err = np.abs(got - want[None]).max(axis=(0, 2))
    print("f64 %s impulses: largest error / budget %.3g, budgets %.3g .. %.3g, smallest |difference| / budget %.3g" % (
        tag, (err / budgets).max(), budgets.min(), budgets.max(), (np.abs(want).max(1) / budgets).min()))
    assert (err <= budgets).all(), (tag, np.flatnonzero(err > budgets), err, budgets)
    assert (logits[:, -1] == logits[0, -1]).all()  # the zero stack does not care where the head is


def test_ties_play_the_first_maximum():
    _need_gpu()
    _judge_ties("light", *run_ties(light_policy, C.shipped("medium"), TIE_ENVS))
    _judge_ties("full-size", *run_ties(full_policy, C.weight_set("full")[0], 5))


def test_impulses_light_and_full_size():
    _need_gpu()
    for tag, make, ws in (("light", light_policy, "medium"), ("full-size", full_policy, "full")):
        wts, full = C.weight_set(ws)
        pol = make(wts, len(C.impulse_stacks()))
        _judge_impulses(tag, wts, full, run_impulses(pol))
        pol.close()


def test_impulses_through_the_league_list_launch():
    _need_gpu()
    from competitive_rl_amd.league import LeagueEnvWrapper
    from tests.test_hip_league import _env

    st = torch.from_numpy(C.impulse_stacks()).cuda()
    n = len(st)
    lg = LeagueEnvWrapper(_env(n, 2), n, ["RULE_BASED", "MEDIUM"], seed=1)
    lg.record_logits = True
    lg.set_opponents("MEDIUM")
    mine = torch.zeros((n,), dtype=torch.int32, device=lg.device)
    out = []
    for _ in range(4):
        lg.set_stack(torch.roll(st, shifts=1, dims=1))
        lg.prev_opponent_obs = st[:, 3:4].contiguous()
        lg._fill_actions(mine)
        out.append(lg.logits().cpu().numpy().copy())
        assert torch.equal(lg.get_stack(), st)
    _judge_impulses("league list launch", C.shipped("medium"), False, np.stack(out))
    lg.close()


# ---- the superseded kernels of the profiling library
_children = {}


def _child(mode):
    """What tests/policy_f64_child.py gave under CRL_LIB_VARIANT=abl with CRL_POLICY_MFMA=`mode` (None: unset, the default kernel):
    a fresh process per mode, run once per session."""
    if mode not in _children:
        import tempfile

        abl_library()
        env = dict(os.environ, CRL_LIB_VARIANT="abl")
        env.pop("CRL_POLICY_MFMA", None)
        if mode is not None:
            env["CRL_POLICY_MFMA"] = mode
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "child.npz")
            r = subprocess.run([sys.executable, os.path.join(C.ROOT, "tests", "policy_f64_child.py"), out], env=env, capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0 and "policy f64 child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
            with np.load(out) as z:
                _children[mode] = {k: z[k] for k in z.files}
    return _children[mode]


@pytest.mark.parametrize("mode,kernel", [("0", "packed-FMA"), ("1", "fp32-MFMA")])
def test_superseded_kernels(mode, kernel):
    """pong_policy_light_kernel (CRL_POLICY_MFMA=0) and pong_policy_mfma_kernel<false, ...> (=1) in a child process that loads the
    profiling library: every light batch at 7, 13 and 2 059 envs, the ties and the impulses.  Witness that the switch took effect:
    on dense input the logits differ in at least one bit from those of a second child that leaves the switch unset."""
    _need_gpu()
    got, default = _child(mode), _child(None)
    for ws, kind in LIGHT:
        for n in CHILD_SIZES:
            key = "%s__%s__%d__" % (ws, kind, n)
            C.judge(kernel, C.case(ws, kind), got[key + "logits"], got[key + "actions"], n)
    _judge_ties(kernel, got["tie__logits"], got["tie__actions"])
    _judge_impulses(kernel, C.shipped("medium"), False, got["impulse__logits"])
    key = "medium__dense__13__logits"
    assert not np.array_equal(got[key].view(np.int32), default[key].view(np.int32)), "CRL_POLICY_MFMA=%s ran the default kernel" % mode


def test_the_profiling_library_serves_the_default_kernel_unchanged():
    """CRL_POLICY_MFMA unset under the profiling library is the shipped kernel: the same bits as this process computes."""
    _need_gpu()
    default = _child(None)
    c = C.case("medium", "dense")
    pol = light_policy(c.weights, 13)
    lg, act = run_calls(pol, c.frames_for(13))
    pol.close()
    assert np.array_equal(lg.view(np.int32), default["medium__dense__13__logits"].view(np.int32))
    assert np.array_equal(act, default["medium__dense__13__actions"])

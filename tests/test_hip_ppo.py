"""LightPPO (include/crl.h "ppo update", csrc/pong_ppo.hip) on the device, on the rollouts and batches of tests/ppo_cases.py.

1. The gradient of every tensor against float64 autograd within the budget rule of ppo_cases (references only); 7. the statistics by the
same rule.  Measured on an MI355X (docs/LAB_NOTES_ppo_update.md has every batch): the largest error / budget over the six batches is
conv1_w 0.30, conv1_b 0.31, conv2_w 0.37, conv2_b 0.35, actor_w 0.37, actor_b 0.45, critic_w 0.14, critic_b 0.25; statistics: policy 0.14,
value 0.40, entropy 0.14, kl 0.08, clipped 0.  2. The same idx twice: identical bits.  3. A batch of 9 in the zero-gradient branch with
vf = ent = 0: an exactly zero actor gradient.  4. step() against rules.adam_reference fed the device's own gradient and norm, bit for bit, three steps,
a max_grad_norm that clips and one that does not.  5. push() into a Policy and a league slot against a fresh Policy of
learner.weights(), bit for bit.  6. update() against the same explicit grad / step sequence, bit for bit.  8. The host-side refusals.

9. .. 12. ppo_cases.BIG_CASES, (N 67, B 2500): 313 groups on 256 workgroups, so workgroups 0 .. 56 run a SECOND pass over the LDS buffers
with the accumulators, the bias and head sums and the statistics carried over (the last of them on a partial group of 4) -- what every
batch above 2048 samples does and no batch of CASES reaches.  9. The gradients and 10. the statistics and the gradient norm against float64
within the three-reference budget (forward, reverse, seq32); 11. the same idx twice on one learner and on a second one: identical bits,
statistics included (a race between passes shows here first); 12. a batch of 9 on the same learner afterwards: the bits of a fresh
learner (no stale partials when the 256 workgroups become 2).  Measured on an MI355X: the largest error / budget is conv1_w 0.02,
conv1_b 0.01, conv2_w 0.02, conv2_b 0.02, actor_w 0.02, actor_b 0.02, critic_w 0.02, critic_b 0.03; statistics: policy 0.00, value 0.00,
entropy 0.00, kl 0.01, clipped 0."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from competitive_rl_amd import _native as NAT  # noqa: E402
from competitive_rl_amd.ppo import LightPPO  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import PPO_KEYS, adam_reference  # noqa: E402
from tests import ppo_cases as P  # noqa: E402
from tests.policy_f64_child import full_policy, light_policy  # noqa: E402
from tests.policy_full_weights import make_weights  # noqa: E402


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in PPO_KEYS)


_storages, _runs = {}, {}


def storage(n):
    """the rollout of ppo_cases.rollout(n) recorded into a RolloutStorage, once per process"""
    if n not in _storages:
        st = RolloutStorage(P.T, n, normalize_advantage=True)
        P.rollout(n).fill(st)
        _storages[n] = st
    return _storages[n]


def learner(**hyper):
    return LightPPO(P.chosen()[1], **{**P.HYPER, **hyper})


def _host(grads):
    return {k: grads[k].cpu().numpy().copy() for k in PPO_KEYS}


def run(n, b):
    """(the device's gradients, its statistics) of batch (n, b), once per process"""
    if (n, b) not in _runs:
        bt = P.chosen()[2][(n, b)]
        lr = learner()
        g = _host(lr.grad(storage(n), torch.from_numpy(bt.idx.astype(np.int64)).cuda()))
        _runs[(n, b)] = (g, lr.stats())
        lr.close()
    return _runs[(n, b)]


@pytest.mark.parametrize("n,b", P.CASES)
def test_gradients_against_float64(n, b):
    _need_gpu()
    bt = P.chosen()[2][(n, b)]
    g, _ = run(n, b)
    err = P.rel_err(g, bt.r64["grads"])
    print("ppo grad N %d B %d: " % (n, b) + "  ".join("%s err %.3g budget %.3g (%.2f)" % (k, err[k], bt.budget[k], err[k] / bt.budget[k]) for k in PPO_KEYS))
    for k in PPO_KEYS:
        assert g[k].shape == bt.r64["grads"][k].shape and err[k] <= bt.budget[k], (k, err[k], bt.budget[k])


@pytest.mark.parametrize("n,b", P.CASES)
def test_statistics_against_float64(n, b):
    _need_gpu()
    bt = P.chosen()[2][(n, b)]
    g, st = run(n, b)
    got = dict(zip(P.STAT_KEYS, st[:5]))
    print("ppo stats N %d B %d: " % (n, b) + "  ".join("%s %.6g err %.3g budget %.3g" % (k, got[k], abs(got[k] - bt.r64[k]), bt.stat_budget[k]) for k in P.STAT_KEYS))
    for k in P.STAT_KEYS:
        assert abs(got[k] - bt.r64[k]) <= bt.stat_budget[k], (k, got[k], bt.r64[k], bt.stat_budget[k])
    sq = sum(float((g[k].astype(np.float64) ** 2).sum()) for k in PPO_KEYS)
    assert abs(st.grad_norm - np.sqrt(sq)) <= 1e-12 * np.sqrt(sq) and st.steps == 0


@pytest.mark.parametrize("n,b", [(1, 7), (67, 130)])
def test_the_same_idx_gives_the_same_bits(n, b):
    """twice on one learner, and once more on a second learner object"""
    _need_gpu()
    idx = torch.from_numpy(P.chosen()[2][(n, b)].idx.astype(np.int64)).cuda()
    first, _ = run(n, b)
    lr = learner()
    for _ in range(2):
        assert _same_bits(_host(lr.grad(storage(n), idx)), first)
    lr.close()


def test_zero_gradient_branch_gives_an_exactly_zero_actor_gradient():
    """B = 9, one step of 9 envs whose every done is set, so the advantage is reward - value exactly: samples with r = 1.5 get A = +1,
    samples with r = 0.5 get A = -1 (the stored log-prob sets r), vf = ent = 0"""
    _need_gpu()
    n = 9
    rs = np.random.RandomState(77)
    w = P.chosen()[1]
    stack = rs.randint(1, 256, (n, 4, 42, 42)).astype(np.uint8)
    frame = rs.randint(0, 256, (n, 42, 42)).astype(np.uint8)
    stacks = np.concatenate([stack[:, 1:], frame[:, None]], axis=1)
    actions = (np.arange(n) % 3).astype(np.int32)
    zero = np.zeros(n, np.float32)
    logp = P.ppo_loss_reference(w, stacks, actions, zero, zero, zero)["logp"]
    up = np.arange(n) % 2 == 0
    old = (logp - np.log(np.where(up, 1.5, 0.5))).astype(np.float32)
    adv = np.where(up, 1.0, -1.0).astype(np.float32)
    values = (rs.randint(-16, 17, n) / 8.0).astype(np.float32)  # (multiples of 1/8: values + adv and back are exact in float32)
    rewards = (values + adv).astype(np.float32)
    assert np.array_equal((rewards - values).astype(np.float32), adv)
    hyper = dict(clip=0.2, vf_coef=0.0, ent_coef=0.0)
    ref = P.ppo_loss_reference(w, stacks, actions, old, rewards, adv, hyper)
    assert not ref["active"].any() and all(not ref["grads"][k].any() for k in PPO_KEYS)
    st = RolloutStorage(1, n, normalize_advantage=False)
    st.begin(torch.from_numpy(stack).cuda())
    st.record(torch.from_numpy(frame[:, None]).cuda(), None, torch.from_numpy(values).cuda(), torch.from_numpy(actions).cuda(), torch.from_numpy(old).cuda())
    st.outcome(torch.from_numpy(rewards).cuda(), torch.ones(n, dtype=torch.uint8, device="cuda"))
    st.finish()
    lr = LightPPO(w, **hyper)
    g = _host(lr.grad(st, torch.from_numpy(rs.permutation(n).astype(np.int64)).cuda()))
    assert not g["actor_w"].any() and not g["actor_b"].any()
    assert all(not g[k].any() for k in PPO_KEYS)  # (vf = 0: nothing else flows either)
    assert lr.stats().clip_fraction == 1.0
    lr.close(), st.close()


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_step_is_the_written_adam_bit_for_bit(max_norm):
    _need_gpu()
    n, b = 67, 130
    idx = torch.from_numpy(P.chosen()[2][(n, b)].idx.astype(np.int64)).cuda()
    hyper = dict(lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=max_norm)
    lr = learner(**hyper)
    p = lr.weights()
    assert _same_bits(p, P.chosen()[1])
    m, v = {k: np.zeros_like(p[k]) for k in PPO_KEYS}, {k: np.zeros_like(p[k]) for k in PPO_KEYS}
    for step in (1, 2, 3):
        g = _host(lr.grad(storage(n), idx))
        norm = lr.stats().grad_norm
        assert (norm > max_norm) == (max_norm == 0.5), norm
        lr.step()
        for k in PPO_KEYS:
            p[k], m[k], v[k] = adam_reference(p[k], m[k], v[k], g[k], norm, step, hyper)
        got = lr.weights()
        assert _same_bits(got, p), step
        assert lr.stats().steps == step
    assert not _same_bits(p, P.chosen()[1])
    lr.close()


def _stepped_learner():
    lr = learner()
    lr.grad(storage(11), torch.from_numpy(P.chosen()[2][(11, 9)].idx.astype(np.int64)).cuda())
    lr.step()
    return lr


def test_push_into_a_policy_serves_the_learners_weights():
    _need_gpu()
    n = 11
    rs = np.random.RandomState(8)
    lr = _stepped_learner()
    pol = light_policy(P.base_weights(), n)
    frames = rs.randint(0, 256, (3, n, 1, 42, 42)).astype(np.uint8)
    pol.act_rollout(torch.from_numpy(frames[0]).cuda())
    lr.push(pol)
    w = lr.weights()
    assert not _same_bits(w, P.base_weights())
    twin = light_policy(w, n)
    twin.act_rollout(torch.from_numpy(frames[0]).cuda())
    for t in (1, 2):
        out = []
        for q in (pol, twin):
            val, act, logp = q.act_rollout(torch.from_numpy(frames[t]).cuda(), want_logits=True)
            out.append([x.cpu().numpy().copy() for x in (q.logits(), val, logp)] + [act.cpu().numpy().copy()])
        for a, c in zip(*out):
            assert np.array_equal(a.view(np.int32), c.view(np.int32)), t
    pol.close(), twin.close(), lr.close()


def test_push_into_a_league_slot_serves_the_learners_weights():
    _need_gpu()
    from competitive_rl_amd.league import LeagueEnvWrapper
    from tests.test_hip_league import _env

    n = 13
    rs = np.random.RandomState(9)
    lr = _stepped_learner()
    lg = LeagueEnvWrapper(_env(n, 21), n, ["RULE_BASED", "MEDIUM"], seed=5)
    lg.set_sampling("MEDIUM", 0.0, 0.0)
    lg.record_logits = True
    lg.set_opponents(np.ones(n, np.int64))
    lr.push(lg, "MEDIUM")
    twin = light_policy(lr.weights(), n)
    mine = torch.zeros((n,), dtype=torch.int32, device=lg.device)
    for t in range(2):
        frame = torch.from_numpy(rs.randint(0, 256, (n, 1, 42, 42)).astype(np.uint8)).cuda()
        lg.prev_opponent_obs = frame
        acts = lg._fill_actions(mine)[:, 1].cpu().numpy().copy()
        a = twin.act_device(frame, want_logits=True).cpu().numpy()
        assert np.array_equal(_bits(lg.logits().cpu().numpy()), _bits(twin.logits().cpu().numpy())) and np.array_equal(acts, a), t
    with pytest.raises(NAT.CrlError):
        lr.push(lg, "RULE_BASED")
    twin.close(), lr.close(), lg.close()


def test_update_is_the_explicit_grad_and_step_sequence():
    _need_gpu()
    n, epochs, batches = 11, 2, 3
    st = storage(n)
    a, b = learner(), learner()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(123)
    a.update(st, epochs, batches, generator=gen)
    gen.manual_seed(123)
    total = P.T * n
    size = total // batches
    for _ in range(epochs):
        perm = torch.randperm(total, device="cuda", generator=gen)
        for k in range(batches):
            b.grad(st, perm[k * size:(k + 1) * size])
            b.step()
    assert _same_bits(a.weights(), b.weights()) and a.stats().steps == epochs * batches == b.stats().steps
    assert not _same_bits(a.weights(), P.chosen()[1])
    a.close(), b.close()


def test_host_side_refusals():
    _need_gpu()
    lr = learner()
    L, hyper = lr._L, lr._hyper()
    stream = lr._stream()
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    ip = ctypes.c_void_p(idx.data_ptr())
    fresh = RolloutStorage(P.T, 3)
    with pytest.raises(NAT.CrlError, match="not finished"):
        lr.grad(fresh, idx)
    st = storage(11)
    assert L.crl_ppo_grad(lr._h, st._h, ip, 0, ctypes.byref(hyper), stream) == -1 and b"number of samples" in L.crl_last_error()
    assert L.crl_ppo_grad(lr._h, st._h, ip, -3, ctypes.byref(hyper), stream) == -1
    assert L.crl_ppo_grad(lr._h, st._h, None, 8, ctypes.byref(hyper), stream) == -1 and b"null" in L.crl_last_error()
    assert L.crl_ppo_grad(lr._h, None, ip, 8, ctypes.byref(hyper), stream) == -1
    assert L.crl_ppo_step(lr._h, ctypes.byref(hyper), stream) == -1 and b"no gradient" in L.crl_last_error()
    full = full_policy(make_weights(5), 3)
    with pytest.raises(NAT.CrlError, match="full-size"):
        lr.push(full)
    with pytest.raises(ValueError, match="critic"):
        LightPPO({k: v for k, v in P.base_weights().items() if not k.startswith("critic")})
    full.close(), fresh.close(), lr.close()


# ---- 9. .. 12. BIG_CASES: 313 groups on 256 workgroups, so workgroups 0 .. 56 run a second pass (the last of them on a partial group)
def big_run(n, b):
    """(the device's gradients, its statistics) of big batch (n, b), once per process"""
    if (n, b) not in _runs:
        lr = learner()
        g = _host(lr.grad(storage(n), torch.from_numpy(P.big()[(n, b)].idx.astype(np.int64)).cuda()))
        _runs[(n, b)] = (g, lr.stats())
        lr.close()
    return _runs[(n, b)]


@pytest.mark.parametrize("n,b", P.BIG_CASES)
def test_big_batch_gradients_against_float64(n, b):
    _need_gpu()
    bt = P.big()[(n, b)]
    g, _ = big_run(n, b)
    err = P.rel_err(g, bt.r64["grads"])
    print("ppo grad N %d B %d: " % (n, b) + "  ".join("%s err %.3g budget %.3g (%.2f)" % (k, err[k], bt.budget[k], err[k] / bt.budget[k]) for k in PPO_KEYS))
    for k in PPO_KEYS:
        assert g[k].shape == bt.r64["grads"][k].shape and err[k] <= bt.budget[k], (k, err[k], bt.budget[k])


@pytest.mark.parametrize("n,b", P.BIG_CASES)
def test_big_batch_statistics_against_float64(n, b):
    _need_gpu()
    bt = P.big()[(n, b)]
    g, st = big_run(n, b)
    got = dict(zip(P.STAT_KEYS, st[:5]))
    print("ppo stats N %d B %d: " % (n, b) + "  ".join("%s %.6g err %.3g budget %.3g (%.2f)" % (k, got[k], abs(got[k] - bt.r64[k]), bt.stat_budget[k],
                                                                                                 abs(got[k] - bt.r64[k]) / bt.stat_budget[k]) for k in P.STAT_KEYS))
    for k in P.STAT_KEYS:
        assert abs(got[k] - bt.r64[k]) <= bt.stat_budget[k], (k, got[k], bt.r64[k], bt.stat_budget[k])
    sq = sum(float((g[k].astype(np.float64) ** 2).sum()) for k in PPO_KEYS)
    assert abs(st.grad_norm - np.sqrt(sq)) <= 1e-12 * np.sqrt(sq) and st.steps == 0


@pytest.mark.parametrize("n,b", P.BIG_CASES)
def test_big_batch_gives_the_same_bits_and_leaves_nothing_behind(n, b):
    """the big batch twice on one learner and against a second learner (the cached run): identical bits, statistics included; then a
    batch of 9 on the same learner -- two workgroups where there were 256 -- gives the bits of a fresh learner"""
    _need_gpu()
    idx = torch.from_numpy(P.big()[(n, b)].idx.astype(np.int64)).cuda()
    first, stats = big_run(n, b)
    lr = learner()
    for _ in range(2):
        assert _same_bits(_host(lr.grad(storage(n), idx)), first) and lr.stats() == stats
    small, small_stats = run(11, 9)
    assert _same_bits(_host(lr.grad(storage(11), torch.from_numpy(P.chosen()[2][(11, 9)].idx.astype(np.int64)).cuda())), small) and lr.stats() == small_stats
    lr.close()

"""FullPPO (include/crl.h "ppo update, full size", csrc/pong_ppo_full.hip) on the device, on the rollouts and batches of
tests/ppo_full_cases.py.

1. The gradient of all ten tensors against float64 autograd within the budget rule of ppo_full_cases (references only), for every case at
the default scratch_rows and for (67, 130) with scratch_rows = 64 (three chunks, the last of two rows; 130 also crosses a 128-row tile);
2. the statistics and the gradient norm by the same rule.  3. The same idx gives the same bits: twice on one learner, on a second learner,
and chunked.  4. A batch of 9 in the zero-gradient branch with vf = ent = 0: all ten tensors exactly zero.  5. step() against
rules.adam_reference fed the device's own gradient and norm, bit for bit, three steps, a max_grad_norm that clips and one that does not, pads
zero.  6. set_weights then grad equals a fresh learner's gradient, bit for bit.  7. push() into a full-size Policy and a league's full-size
slot against a fresh Policy of learner.weights(), bit for bit.  8. update() against the explicit grad / step sequence.  9. The host-side
refusals.

Measured on an MI355X (docs/LAB_NOTES_ppo_full_update.md has every batch): the largest error / budget over the seven runs is
conv1_w 0.08, conv1_b 0.05, conv2_w 0.12, conv2_b 0.11, conv3_w 0.12, conv3_b 0.24, actor_w 0.11, actor_b 0.12, critic_w 0.11, critic_b 0.28;
statistics: policy 0.06, value 0.04, entropy 0.17, kl 0.26, clipped 0.00.

10. .. 13. ppo_full_cases.BIG_CASES, (N 67, B 601), at the default scratch_rows (one chunk: the back kernel's workgroups 0 .. 88 take three
rows and the rest two with gW1, gW2, gb1, gb2 held across them; three head slices 256 + 256 + 89; the front kernel's row loop; a last
heads workgroup of one row) and at scratch_rows = BIG_ROWS = 320 (chunks of 320 and 281, each of two slices with a partial second one,
the second chunk adding onto the first one's sums: ``first == 0`` with ``slices > 1``) -- what production's 64 rows per workgroup and
64 slices per chunk do and no batch of CASES reaches.  10. The gradients and 11. the statistics and the gradient norm against float64
within the three-reference budget (forward, reverse, seq32); 12. the same idx twice on one learner and on a second one: identical bits,
statistics included; 13. a batch of 9 on the same learner afterwards: the bits of a fresh learner.  Measured on an MI355X: the largest
error / budget over the two runs is conv1_w 0.03, conv1_b 0.02, conv2_w 0.06, conv2_b 0.03, conv3_w 0.11, conv3_b 0.09, actor_w 0.05,
actor_b 0.04, critic_w 0.03, critic_b 0.03; statistics: policy 0.01, value 0.02, entropy 0.00, kl 0.00, clipped 0.00."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from competitive_rl_amd import _native as NAT  # noqa: E402
from competitive_rl_amd.ppo import FULL_BLOB_FLOATS, FULL_BLOB_LAYOUT, FullPPO, LightPPO  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import PPO_FULL_KEYS as KEYS  # noqa: E402
from competitive_rl_amd.rules import adam_reference, ppo_full_loss_reference  # noqa: E402
from tests import ppo_cases as PL  # noqa: E402
from tests import ppo_full_cases as P  # noqa: E402
from tests.policy_f64_child import full_policy, light_policy  # noqa: E402

CHUNKED = 64  # scratch_rows of the chunked configuration
RUNS = [(n, b, None) for n, b in P.CASES] + [(67, 130, CHUNKED)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


_storages, _runs = {}, {}


def storage(n):
    """the rollout of ppo_full_cases.rollout(n) recorded into a RolloutStorage, once per process"""
    if n not in _storages:
        st = RolloutStorage(P.T, n, normalize_advantage=True)
        P.rollout(n).fill(st)
        _storages[n] = st
    return _storages[n]


def learner(scratch_rows=None, weights=None, **hyper):
    return FullPPO(P.chosen()[1] if weights is None else weights, scratch_rows=scratch_rows, **{**P.HYPER, **hyper})


def _host(grads):
    return {k: grads[k].cpu().numpy().copy() for k in KEYS}


def _idx(n, b):
    return torch.from_numpy(P.chosen()[2][(n, b)].idx.astype(np.int64)).cuda()


def run(n, b, rows=None):
    """(the device's gradients, its statistics) of batch (n, b) at scratch_rows `rows`, once per process"""
    if (n, b, rows) not in _runs:
        lr = learner(rows)
        g = _host(lr.grad(storage(n), _idx(n, b)))
        _runs[(n, b, rows)] = (g, lr.stats())
        lr.close()
    return _runs[(n, b, rows)]


@pytest.mark.parametrize("n,b,rows", RUNS)
def test_gradients_against_float64(n, b, rows):
    _need_gpu()
    bt = P.chosen()[2][(n, b)]
    g, _ = run(n, b, rows)
    err = P.rel_err(g, bt.r64["grads"])
    print("ppo full grad N %d B %d rows %s: " % (n, b, rows) + "  ".join("%s err %.3g budget %.3g (%.2f)" % (k, err[k], bt.budget[k], err[k] / bt.budget[k]) for k in KEYS))
    for k in KEYS:
        assert g[k].shape == bt.r64["grads"][k].shape and err[k] <= bt.budget[k], (k, err[k], bt.budget[k])


@pytest.mark.parametrize("n,b,rows", RUNS)
def test_statistics_against_float64(n, b, rows):
    _need_gpu()
    bt = P.chosen()[2][(n, b)]
    g, st = run(n, b, rows)
    got = dict(zip(P.STAT_KEYS, st[:5]))
    print("ppo full stats N %d B %d rows %s: " % (n, b, rows) + "  ".join("%s %.6g err %.3g budget %.3g" % (k, got[k], abs(got[k] - bt.r64[k]), bt.stat_budget[k]) for k in P.STAT_KEYS))
    for k in P.STAT_KEYS:
        assert abs(got[k] - bt.r64[k]) <= bt.stat_budget[k], (k, got[k], bt.r64[k], bt.stat_budget[k])
    sq = sum(float((g[k].astype(np.float64) ** 2).sum()) for k in KEYS)
    assert abs(st.grad_norm - np.sqrt(sq)) <= 1e-12 * np.sqrt(sq) and st.steps == 0


@pytest.mark.parametrize("n,b,rows", [(1, 7, None), (67, 130, None), (67, 130, CHUNKED)])
def test_the_same_idx_gives_the_same_bits(n, b, rows):
    """twice on one learner, and once more on a second learner object (the cached run)"""
    _need_gpu()
    first, _ = run(n, b, rows)
    lr = learner(rows)
    for _ in range(2):
        assert _same_bits(_host(lr.grad(storage(n), _idx(n, b))), first)
    lr.close()


def test_zero_gradient_branch_gives_exactly_zero_gradients():
    """B = 9, one step of 9 envs whose every done is set, so the advantage is reward - value exactly: samples with r = 1.5 get A = +1,
    samples with r = 0.5 get A = -1 (the stored log-prob sets r), vf = ent = 0.  The learner has run another batch before, so scratch and
    accumulators hold other values."""
    _need_gpu()
    n = 9
    rs = np.random.RandomState(77)
    w = P.chosen()[1]
    stack = rs.randint(1, 256, (n, 4, 42, 42)).astype(np.uint8)
    frame = rs.randint(0, 256, (n, 42, 42)).astype(np.uint8)
    stacks = np.concatenate([stack[:, 1:], frame[:, None]], axis=1)
    actions = (np.arange(n) % 3).astype(np.int32)
    zero = np.zeros(n, np.float32)
    logp = ppo_full_loss_reference(w, stacks, actions, zero, zero, zero)["logp"]
    up = np.arange(n) % 2 == 0
    old = (logp - np.log(np.where(up, 1.5, 0.5))).astype(np.float32)
    adv = np.where(up, 1.0, -1.0).astype(np.float32)
    values = (rs.randint(-16, 17, n) / 8.0).astype(np.float32)  # (multiples of 1/8: values + adv and back are exact in float32)
    rewards = (values + adv).astype(np.float32)
    assert np.array_equal((rewards - values).astype(np.float32), adv)
    hyper = dict(clip=0.2, vf_coef=0.0, ent_coef=0.0)
    ref = ppo_full_loss_reference(w, stacks, actions, old, rewards, adv, hyper)
    assert not ref["active"].any() and all(not ref["grads"][k].any() for k in KEYS)
    st = RolloutStorage(1, n, normalize_advantage=False)
    st.begin(torch.from_numpy(stack).cuda())
    st.record(torch.from_numpy(frame[:, None]).cuda(), None, torch.from_numpy(values).cuda(), torch.from_numpy(actions).cuda(), torch.from_numpy(old).cuda())
    st.outcome(torch.from_numpy(rewards).cuda(), torch.ones(n, dtype=torch.uint8, device="cuda"))
    st.finish()
    lr = FullPPO(w, **P.HYPER)
    assert any(v.any() for v in _host(lr.grad(storage(11), _idx(11, 9))).values())
    lr.hyper.update(hyper)
    g = _host(lr.grad(st, torch.from_numpy(rs.permutation(n).astype(np.int64)).cuda()))
    assert all(not g[k].any() for k in KEYS)
    assert lr.stats().clip_fraction == 1.0 and lr.stats().grad_norm == 0.0
    lr.close(), st.close()


def _flat(w):
    out = np.zeros(FULL_BLOB_FLOATS, np.float32)
    for k, (o, s) in FULL_BLOB_LAYOUT.items():
        out[o:o + int(np.prod(s))] = w[k].reshape(-1)
    return out


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_step_is_the_written_adam_bit_for_bit(max_norm):
    _need_gpu()
    n, b = 67, 130
    idx = _idx(n, b)
    hyper = dict(lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=max_norm)
    lr = learner(**hyper)
    p = lr.weights()
    assert _same_bits(p, P.chosen()[1])
    m, v = {k: np.zeros_like(p[k]) for k in KEYS}, {k: np.zeros_like(p[k]) for k in KEYS}
    for step in (1, 2, 3):
        g = _host(lr.grad(storage(n), idx))
        norm = lr.stats().grad_norm
        assert (norm > max_norm) == (max_norm == 0.5), norm
        lr.step()
        for k in KEYS:
            p[k], m[k], v[k] = adam_reference(p[k], m[k], v[k], g[k], norm, step, hyper)
        got = lr.weights()
        assert _same_bits(got, p), step
        assert lr.stats().steps == step
    assert not _same_bits(p, P.chosen()[1])
    # the pads: zero in the weights (the device blob against the tensors alone) and in the gradient
    ptr = ctypes.c_void_p()
    NAT.check(lr._L.crl_ppo_weights_dev(lr._h, ctypes.byref(ptr)))
    assert np.array_equal(_bits(lr._dev_blob(ptr.value).cpu().numpy()), _bits(_flat(p)))
    gh = np.zeros(FULL_BLOB_FLOATS, np.float32)
    NAT.check(lr._L.crl_ppo_get_grad(lr._h, None, gh.ctypes.data_as(ctypes.c_void_p)))
    assert np.array_equal(_bits(gh), _bits(_flat(g)))
    lr.close()


def test_set_weights_then_grad_is_a_fresh_learners_gradient():
    _need_gpu()
    n, b = 11, 9
    w2 = P.perturbed(P.base_weights(), 0.5, seed=9)
    lr = learner()
    lr.grad(storage(n), _idx(n, b))
    lr.step()
    lr.set_weights(w2)
    assert lr.stats().steps == 0 and _same_bits(lr.weights(), w2)
    got = _host(lr.grad(storage(n), _idx(n, b)))
    fresh = learner(weights=w2)
    want = _host(fresh.grad(storage(n), _idx(n, b)))
    assert _same_bits(got, want) and any(want[k].any() for k in KEYS)
    lr.step(), fresh.step()  # (the moments and the step count started over too)
    assert _same_bits(lr.weights(), fresh.weights())
    lr.close(), fresh.close()


def _stepped_learner():
    lr = learner()
    lr.grad(storage(11), _idx(11, 9))
    lr.step()
    return lr


def test_push_into_a_policy_serves_the_learners_weights():
    _need_gpu()
    n = 11
    rs = np.random.RandomState(8)
    lr = _stepped_learner()
    pol = full_policy(P.base_weights(), n)
    frames = rs.randint(0, 256, (3, n, 1, 42, 42)).astype(np.uint8)
    pol.act_rollout(torch.from_numpy(frames[0]).cuda())
    lr.push(pol)
    w = lr.weights()
    assert not _same_bits(w, P.base_weights())
    twin = full_policy(w, n)
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
    lg.add_full_agent("BIG", P.base_weights())
    lg.record_logits = True
    lg.set_opponents(np.full(n, 2, np.int64))
    lr.push(lg, "BIG")
    twin = full_policy(lr.weights(), n)
    mine = torch.zeros((n,), dtype=torch.int32, device=lg.device)
    for t in range(2):
        frame = torch.from_numpy(rs.randint(0, 256, (n, 1, 42, 42)).astype(np.uint8)).cuda()
        lg.prev_opponent_obs = frame
        acts = lg._fill_actions(mine)[:, 1].cpu().numpy().copy()
        a = twin.act_device(frame, want_logits=True).cpu().numpy()
        assert np.array_equal(_bits(lg.logits().cpu().numpy()), _bits(twin.logits().cpu().numpy())) and np.array_equal(acts, a), t
    with pytest.raises(NAT.CrlError, match="LightActorCritic slot"):
        lr.push(lg, "MEDIUM")
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
    full, light = learner(), LightPPO(PL.base_weights())
    L = full._L
    w10 = [np.zeros(s, np.float32).ctypes.data_as(ctypes.c_void_p) for _, s in FULL_BLOB_LAYOUT.values()]
    w8 = w10[:8]  # (pointers only: every call below is refused before it reads one)
    assert L.crl_ppo_set_weights(full._h, *w8) == -1 and b"full-size learner" in L.crl_last_error()
    assert L.crl_ppo_get_weights(full._h, *w8) == -1 and b"full-size learner" in L.crl_last_error()
    assert L.crl_ppo_set_weights_full(light._h, *w10) == -1 and b"LightActorCritic learner" in L.crl_last_error()
    assert L.crl_ppo_get_weights_full(light._h, *w10) == -1 and b"LightActorCritic learner" in L.crl_last_error()
    assert L.crl_ppo_set_weights_full(full._h, *w10[:9], None) == -1 and b"null" in L.crl_last_error()
    h = ctypes.c_void_p()
    assert L.crl_ppo_create_full(0, -1, *w10, ctypes.byref(h)) == -1 and b"scratch_rows" in L.crl_last_error()
    assert L.crl_ppo_create_full(0, 63, *w10, ctypes.byref(h)) == -1 and b"scratch_rows" in L.crl_last_error()
    assert L.crl_ppo_create_full(0, 0, *w10[:9], None, ctypes.byref(h)) == -1 and b"critic" in L.crl_last_error()
    stream = full._stream()
    assert L.crl_ppo_step(full._h, ctypes.byref(full._hyper()), stream) == -1 and b"no gradient" in L.crl_last_error()
    fresh = RolloutStorage(P.T, 3)
    with pytest.raises(NAT.CrlError, match="not finished"):
        full.grad(fresh, torch.zeros(8, dtype=torch.int64, device="cuda"))
    small, big = light_policy(PL.base_weights(), 3), full_policy(P.base_weights(), 3)
    with pytest.raises(NAT.CrlError, match="LightActorCritic policy"):
        full.push(small)
    with pytest.raises(NAT.CrlError, match="full-size"):
        light.push(big)
    assert L.crl_policy_load_full_dev(big._h, None, stream) == -1 and b"null" in L.crl_last_error()
    assert L.crl_pool_load_full_dev(None, 0, None, stream) == -1 and b"null" in L.crl_last_error()
    with pytest.raises(ValueError, match="critic"):
        FullPPO({k: v for k, v in P.base_weights().items() if not k.startswith("critic")})
    with pytest.raises(ValueError, match="full-size ActorCritic"):
        FullPPO(PL.base_weights())
    with pytest.raises(ValueError, match="LightActorCritic"):
        FullPPO(small)
    with pytest.raises(ValueError, match="LightPPO trains the LightActorCritic"):
        LightPPO(big)
    with pytest.raises(TypeError, match="FullPPO takes"):
        FullPPO(P.base_weights(), momentum=0.9)
    small.close(), big.close(), fresh.close(), full.close(), light.close()


# ---- 10. .. 13. BIG_CASES: B = 601 in one chunk (three rows per back workgroup, three head slices, the front kernel's row loop) and in
# chunks of BIG_ROWS (two chunks of two slices each, the second chunk adding onto the first one's sums)
BIG_RUNS = [(n, b, rows) for n, b in P.BIG_CASES for rows in (None, P.BIG_ROWS)]


def _big_idx(n, b):
    return torch.from_numpy(P.big()[(n, b)].idx.astype(np.int64)).cuda()


def big_run(n, b, rows):
    """(the device's gradients, its statistics) of big batch (n, b) at scratch_rows `rows`, once per process"""
    if (n, b, rows) not in _runs:
        lr = learner(rows)
        g = _host(lr.grad(storage(n), _big_idx(n, b)))
        _runs[(n, b, rows)] = (g, lr.stats())
        lr.close()
    return _runs[(n, b, rows)]


@pytest.mark.parametrize("n,b,rows", BIG_RUNS)
def test_big_batch_gradients_against_float64(n, b, rows):
    _need_gpu()
    bt = P.big()[(n, b)]
    g, _ = big_run(n, b, rows)
    err = P.rel_err(g, bt.r64["grads"])
    print("ppo full grad N %d B %d rows %s: " % (n, b, rows) + "  ".join("%s err %.3g budget %.3g (%.2f)" % (k, err[k], bt.budget[k], err[k] / bt.budget[k]) for k in KEYS))
    for k in KEYS:
        assert g[k].shape == bt.r64["grads"][k].shape and err[k] <= bt.budget[k], (k, err[k], bt.budget[k])


@pytest.mark.parametrize("n,b,rows", BIG_RUNS)
def test_big_batch_statistics_against_float64(n, b, rows):
    _need_gpu()
    bt = P.big()[(n, b)]
    g, st = big_run(n, b, rows)
    got = dict(zip(P.STAT_KEYS, st[:5]))
    print("ppo full stats N %d B %d rows %s: " % (n, b, rows) + "  ".join("%s %.6g err %.3g budget %.3g (%.2f)" % (
        k, got[k], abs(got[k] - bt.r64[k]), bt.stat_budget[k], abs(got[k] - bt.r64[k]) / bt.stat_budget[k]) for k in P.STAT_KEYS))
    for k in P.STAT_KEYS:
        assert abs(got[k] - bt.r64[k]) <= bt.stat_budget[k], (k, got[k], bt.r64[k], bt.stat_budget[k])
    sq = sum(float((g[k].astype(np.float64) ** 2).sum()) for k in KEYS)
    assert abs(st.grad_norm - np.sqrt(sq)) <= 1e-12 * np.sqrt(sq) and st.steps == 0


@pytest.mark.parametrize("n,b,rows", BIG_RUNS)
def test_big_batch_gives_the_same_bits_and_leaves_nothing_behind(n, b, rows):
    """the big batch twice on one learner and against a second learner (the cached run): identical bits, statistics included; then a
    batch of 9 on the same learner -- nine back workgroups and one slice where there were 256 and three -- gives the bits of a fresh
    learner of the same scratch_rows"""
    _need_gpu()
    first, stats = big_run(n, b, rows)
    lr, fresh = learner(rows), learner(rows)
    for _ in range(2):
        assert _same_bits(_host(lr.grad(storage(n), _big_idx(n, b))), first) and lr.stats() == stats
    want = _host(fresh.grad(storage(11), _idx(11, 9)))
    assert _same_bits(_host(lr.grad(storage(11), _idx(11, 9))), want) and lr.stats() == fresh.stats() and any(want[k].any() for k in KEYS)
    lr.close(), fresh.close()

"""What the server served, into the learner: ``Policy.act_rollout`` recorded into a ``RolloutStorage`` and handed to ``LightPPO`` /
``FullPPO`` AT THE SERVED WEIGHTS (include/crl.h "ppo update": the learner's forward pass is a sibling of the served kernels, so its
log-probabilities agree with the served ones "to within float32 rounding, not bit for bit").

A Policy of N = 67 envs with set_sampling(1.0, 0.0, seed) plays T = 6 act_rollout calls on random byte frames under the "random" reset
pattern (the loop of test_hip_rollout_storage._play_rollout, the frames kept on the host); finish with normalised advantages; a learner
from the same weights.  The T N samples are screened for ReLU kinks from the host-known stacks (rules.rollout_stack_reference) and the
weights alone: a sample with a pre-activation |z| < 4 x the largest deviation of the two float32 references from float64 is dropped, at
most 20 % of them, at least 300 kept (the full-size run stays above one head slice and one row per back workgroup).

The reference is rules.ppo(_full)_loss_reference in float64, fed the batch that ``storage.gather(idx, obs_dtype=torch.uint8)`` hands
out: the SERVED log-probs, actions, returns and advantages are its inputs.

(a) every gradient tensor and statistic within the three-reference budget of tests/ppo_cases.py (forward, reverse, seq32);
(b) clip_fraction == 0.0 on the device and in the reference: the ratio is 1 to within rounding;
(c) the reference's own kl -- the mean of served log-prob - float64 log-prob -- within
        2 x budget_logits + 8 float32 ulps of max(1, largest |log-prob|):
    the served logits lie within budget_logits of float64 (the rule of tests/policy_f64_cases.py on these stacks: FACTOR x e_ref over its
    BLAS-order and sequential float32 forward passes, at least 2 ulps of the largest |logit|); a log-probability is l_a - logsumexp(l),
    so logits off by at most beta move it by at most 2 beta; and the served log-prob is within 8 ulps of the written rule on the served
    logits (tests/test_hip_rollout.py; the float32 subtraction l_a - max in that rule is under one of those ulps and sits inside the
    doubling its derivation ends with).  Every sample obeys the bound, so their mean does.
A server and a learner that disagree on the temperature, the action index, the / 255 or the reset mask fail (b) or (c) by orders of
magnitude."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from competitive_rl_amd.ppo import FullPPO, LightPPO  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import PPO_FULL_KEYS, PPO_KEYS, ppo_full_loss_reference, ppo_loss_reference, rollout_stack_reference  # noqa: E402
from tests import policy_f64_cases as C  # noqa: E402
from tests import ppo_cases as PL  # noqa: E402
from tests import ppo_full_cases as PF  # noqa: E402
from tests.policy_f64_child import full_policy, light_policy  # noqa: E402
from tests.test_rollout_storage_rules import reset_pattern  # noqa: E402

T, N = 6, 67
DROP_CAP, KEEP_AT_LEAST = 0.20, 300
LOGP_ULPS = 8  # tests/test_hip_rollout.py: the served log-prob against rules.rollout_logp_reference of the served logits


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _play(pol, st, flags, rs):
    """T act_rollout calls recorded into `st`; returns the frames shown, [T, N, 42, 42]"""
    acts2 = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    rew2 = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    frames = rs.randint(0, 256, (T, N, 42, 42)).astype(np.uint8)
    for t in range(T):
        obs = torch.from_numpy(frames[t][:, None]).cuda()
        reset = torch.from_numpy(flags[t]).cuda()
        if t % 2:
            reset = reset.to(torch.uint8) * 5  # (any non-zero byte)
        values, actions, logp = pol.act_rollout(obs, reset=reset, out=acts2[:, 0])
        st.record(obs, reset, values, actions, logp)
        rew2.copy_(torch.from_numpy(rs.standard_normal((N, 2)).astype(np.float32)))
        st.outcome(rew2[:, 0], torch.from_numpy(rs.random_sample(N) < 0.2).cuda())
    return frames


def _reversed(ref, pre):
    for k in pre + ("ratio", "logp", "v", "logits", "active"):
        ref[k] = ref[k][::-1]
    return ref


@pytest.mark.parametrize("full", [False, True], ids=["light", "full"])
def test_the_served_rollout_through_the_learner_at_the_served_weights(full):
    _need_gpu()
    keys, loss, pre = (PPO_FULL_KEYS, ppo_full_loss_reference, PF.PRE) if full else (PPO_KEYS, ppo_loss_reference, ("z1", "z2"))
    w = PF.base_weights() if full else PL.base_weights()
    seed = 41 + full
    rs = np.random.RandomState(seed)
    pol = (full_policy if full else light_policy)(w, N)
    pol.set_sampling(1.0, 0.0, seed=seed)
    st = RolloutStorage(T, N, normalize_advantage=True)
    st.begin(pol)
    flags = reset_pattern("random", T, N, seed)
    frames = _play(pol, st, flags, rs)
    st.finish(torch.from_numpy(rs.standard_normal(N).astype(np.float32)).cuda())
    lr = (FullPPO if full else LightPPO)(w, **PL.HYPER)

    # ---- the screen: the host-known stacks and the weights alone
    stacks, depth = rollout_stack_reference(np.concatenate([np.zeros((3, N, 42, 42), np.uint8), frames]), flags)
    stacks = stacks.reshape(T * N, 4, 42, 42)
    assert (depth < 4).any() and (depth == 4).any()
    order = rs.permutation(T * N)
    zero = np.zeros(T * N, np.float32)

    def forward(rows, dtype):
        return loss(w, stacks[rows], np.zeros(len(rows), np.int64), zero[:len(rows)], zero[:len(rows)], zero[:len(rows)], PL.HYPER, dtype)

    z64 = forward(order, torch.float64)
    dz = max(float(np.abs(r32[k] - z64[k]).max()) for k in pre
             for r32 in (forward(order, torch.float32), _reversed(forward(order[::-1].copy(), torch.float32), pre)))
    zmin = np.min([np.abs(z64[k]).reshape(T * N, -1).min(1) for k in pre], axis=0)
    idx = order[zmin >= 4 * dz]
    dropped = T * N - len(idx)
    print("learner loop %s: dz %.3g, screening dropped %d of %d samples" % ("full" if full else "light", 4 * dz, dropped, T * N))
    assert dropped <= DROP_CAP * T * N and len(idx) >= KEEP_AT_LEAST, (dropped, len(idx))

    # ---- the device, and the reference on what the storage hands out
    dev = torch.from_numpy(idx.astype(np.int64)).cuda()
    g = {k: v.cpu().numpy().copy() for k, v in lr.grad(st, dev).items()}
    stats = lr.stats()
    batch = [None if x is None else x.cpu().numpy() for x in st.gather(dev, obs_dtype=torch.uint8)]
    obs, actions, served_logp, _, returns, adv = batch
    assert obs.dtype == np.uint8 and np.array_equal(obs, stacks[idx])  # (what the policy was shown is what the host knows)

    def reference(rows, dtype=torch.float64):
        return loss(w, obs[rows], actions[rows], served_logp[rows], returns[rows], adv[rows], PL.HYPER, dtype)

    rows = np.arange(len(idx))
    bt = types.SimpleNamespace(r64=reference(rows))
    PL.set_budgets(bt, (reference(rows, torch.float32), _reversed(reference(rows[::-1].copy(), torch.float32), pre),
                        PL.seq32(lambda one: reference(one, torch.float32), rows, keys, cache=False)), keys)
    assert bt.ref_names[-1] == "seq32" and len(bt.errs) == 3

    # (a)
    err = PL.rel_err(g, bt.r64["grads"], keys)
    got = dict(zip(PL.STAT_KEYS, stats[:5]))
    tag = "learner loop %s B %d: " % ("full" if full else "light", len(idx))
    print(tag + "  ".join("%s err %.3g budget %.3g (%.2f)" % (k, err[k], bt.budget[k], err[k] / bt.budget[k]) for k in keys))
    print(tag + "  ".join("%s %.6g err %.3g budget %.3g (%.2f)" % (k, got[k], abs(got[k] - bt.r64[k]), bt.stat_budget[k],
                                                                   abs(got[k] - bt.r64[k]) / bt.stat_budget[k]) for k in PL.STAT_KEYS))
    # (c)'s figures, printed before anything is asserted
    l64, e_ref, _ = C.references(w, obs, full)
    beta = C.budget_of(l64, e_ref)
    bound = 2 * beta + LOGP_ULPS * C.ulp32(max(1.0, float(np.abs(bt.r64["logp"]).max())))
    worst = float(np.abs(served_logp.astype(np.float64) - bt.r64["logp"]).max())
    print(tag + "reference kl %.3g, largest |served log-prob - float64 log-prob| %.3g, bound %.3g (logits budget %.3g); device kl %.3g" % (
        bt.r64["kl"], worst, bound, beta, got["kl"]))
    for k in keys:
        assert g[k].shape == bt.r64["grads"][k].shape and err[k] <= bt.budget[k], (k, err[k], bt.budget[k])
    for k in PL.STAT_KEYS:
        assert abs(got[k] - bt.r64[k]) <= bt.stat_budget[k], (k, got[k], bt.r64[k], bt.stat_budget[k])
    # (b)
    assert stats.clip_fraction == 0.0 and bt.r64["clipped"] == 0.0 and bt.r64["active"].all()
    # (c)
    assert np.abs(l64 - bt.r64["logits"]).max() <= 1e-12 * np.abs(l64).max()  # (the two float64 forward passes are one network)
    assert abs(bt.r64["kl"]) <= bound, (bt.r64["kl"], bound)
    lr.close(), st.close(), pol.close()

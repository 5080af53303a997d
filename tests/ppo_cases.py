"""Rollouts, batches, the error budget and the fault models shared by tests/test_ppo_rules.py (CPU) and tests/test_hip_ppo.py (GPU): the
device's PPO gradient (include/crl.h "ppo update") against float64 autograd of the written rule (rules.ppo_loss_reference).

Everything here is computed from references alone, never from device output.

ROLLOUTS.  T = 6 steps of N in {1, 11, 67} envs, made up as tests/test_hip_rollout_storage.py's ``Filled`` makes them up (a non-zero
stack in front, uniform random byte frames, uniform random actions, normal rewards, 20 % dones) under a reset pattern, so masked planes
and depths below 4 occur; normalisation on.  The stored log-probs and values are those of the UNPERTURBED shipped ``medium`` weights
(float64 forward, rounded to float32); the learner holds ``medium`` perturbed by AMOUNT x each tensor's standard deviation x a seeded
normal draw.  AMOUNT is the first of AMOUNTS at which, over all kept samples of all batches, at least 10 % lie in the zero-gradient
branch of the clipped ratio, at least 30 % in the other, and all three actions occur.

BATCHES.  (N, B) in CASES, B in {1, 7, 8, 9, 67, 130}: below, at and over one group of 8, over several workgroups.  ``idx`` is drawn
with replacement (shuffled, duplicates).  Gradients of a ReLU net and of the clipped ratio are discontinuous, so candidates are screened
from the float64 reference: a candidate with a pre-activation |z| < dz or with |r - (1 +- c)| < dr is dropped, dz and dr each 4 x the
largest deviation of that quantity from float64 over the two float32 references on the candidates.  At most 10 % of all candidates may
be dropped (test_ppo_rules.py asserts it).

BUDGET, per tensor:  err = max|g - g64| / max|g64|;  e_ref = the larger err of the two float32 references (torch float32 autograd on
the CPU, and the same with the samples in reverse order);  budget = max(FACTOR x e_ref, 2 float32 ulps of 1), the rule of
tests/policy_f64_cases.py.

FACTOR = 10, raised from 2 for a reason measured on the REFERENCES alone: e_ref is not a property of the batch but of the CPU that
evaluates the float32 references.  The same torch float32 autograd on the same batch (N 11, B 8) is off from float64 by 7.8e-6, 6.4e-6,
5.8e-6, 4.8e-6, 1.3e-5, 1.3e-5 (conv1_w .. actor_b) on one x86 host and by 1.29e-6, 9.65e-7, 8.0e-7, 7.0e-7, 1.58e-6, 1.33e-6 on
another: ratios 6.0 .. 9.8; critic_b of (N 1, B 7), one number, 1.1e-6 against 1.88e-7: 5.9.  (Both orders of one host agree with each
other to a few per cent, so the second reference does not see this.)  A budget of 2 x e_ref taken on the second host therefore fails
the first host's float32 reference itself by a factor of up to 4.9.  FACTOR = 10 is the smallest round factor at which the budget
taken on either host admits the float32 reference evaluated on the other, which a check of a float32 kernel has to.  The fault models
stay at least 2 x budget away (test_ppo_rules.py), which is what keeps the wider factor honest; the entropy coefficient of the
test, 0.1, is chosen for that.  docs/LAB_NOTES_ppo_update.md has both hosts' tables and the device's error / budget per tensor.

STATISTICS: absolute errors, the same FACTOR x e_ref; the floor is, for the policy loss, the entropy and the approximate KL, 2 float32
ulps of the batch's largest |logit| -- the floor tests/policy_f64_cases.py gives the logits themselves: these three are functions of
log-probabilities, and a log-probability formed from float32 features cannot be known better than its logits --, and 2 ulps of
max(|statistic|, 1) for the value loss and the clipped share.

BIG_CASES, (N 67, B 2500).  pong_ppo.hip launches W = min(256, ceil(B / 8)) workgroups and workgroup w takes the groups w, w + W, ...: at
B <= 130 every workgroup runs one pass, so nothing in CASES makes a workgroup re-use its LDS buffers or carry its accumulators, bias and
head sums and statistics into a second pass -- which every batch above 2048 samples does (B = 262 144: 128 passes).  2500 is 313 groups:
workgroups 0 .. 56 run two passes, the rest one, and the last group is partial (4 samples) and is a SECOND pass (workgroup 56).  The
batch is built by ``big()`` on rollout(67) at the weights chosen() has chosen, by the same candidate draw and screening (3128
candidates); it takes no part in chosen()'s shares, AMOUNT or the 10 % drop cap over CASES, which come out bit-identical.  Its own cap:
at most BIG_DROP_CAP = 20 % of its candidates dropped (the value ppo_full_cases.DROP_CAP uses; 426 / 3128 = 13.6 %), and it must fill.

SEQ32, the third float32 reference behind the big batches' e_ref: the float32 autograd gradient of each sample's own loss term, added
one sample at a time in idx order into a float32 accumulator, divided by float32(B) at the end; the statistics the same way.  It is the
strictly sequential order (the idea of policy_oracle.forward_seq32), and the shape the headers prescribe for the full-size w3 and head
slices.  Two references are not enough at these sizes: torch's blocked sums over B are nearly exact on the short tensors, so e_ref
over forward and reverse alone describes torch's summation and not float32 summation.  Measured on one x86 host, seq32's error over that
two-reference e_ref: light B 2500 critic_w 7.9, critic_b 3.3, actor_b 2.8, actor_w 2.0; full B 601 critic_b 11.0, conv3_b 6.2, actor_b 3.5,
conv3_w 2.2 -- a CORRECT strictly sequential float32 kernel would fail a two-reference budget on critic_b.  FACTOR stays 10.

FAULT MODELS between passes (BIG_FAULTS, float64): pass_repeats -- a later pass sees its workgroup's previous inputs, so the samples at
positions >= 8 x 256 are those 2048 places earlier; earlier_pass_lost -- a later pass overwrites instead of adding, so only each
workgroup's last pass is left (groups 57 .. 312) and the sum is still divided by B.  test_ppo_rules.py asserts every fault model, old
and new, at least 2 x the three-reference budget away on the big batch.
"""
import math

import numpy as np
import torch

from competitive_rl_amd.rules import PPO_KEYS, gae_reference, ppo_loss_reference, rollout_stack_reference
from tests import policy_f64_cases as C
from tests.test_rollout_storage_rules import reset_pattern

T = 6
FACTOR = 10  # (see above)
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.1)  # (ent_coef: keeps the omitted-entropy fault 2 x budget away on every batch)
CASES = ((1, 1), (1, 7), (11, 8), (11, 9), (67, 67), (67, 130))
BIG_CASES = ((67, 2500),)  # (313 groups on 256 workgroups: see the module docstring)
GROUP, WORKGROUPS = 8, 256  # pong_ppo.hip: samples per group, the most workgroups a launch has
BIG_DROP_CAP = 0.20
PATTERN = {1: "two_consecutive", 11: "random", 67: "random"}
AMOUNTS = (0.002, 0.005, 0.01, 0.02, 0.05, 0.1)
STAT_KEYS = ("policy", "value", "entropy", "kl", "clipped")
ULP1 = 2.0 ** -23


def base_weights():
    z = np.load(C.ROOT + "/competitive_rl_amd/assets/pong_policy_medium.npz")
    return {k: np.ascontiguousarray(z[k], np.float32) for k in PPO_KEYS}


def perturbed(base, amount, seed=5):
    rs = np.random.RandomState(seed)
    return {k: (base[k] + np.float32(amount) * np.float32(base[k].std() if base[k].size > 1 else abs(base[k]).max()) *
                rs.standard_normal(base[k].shape).astype(np.float32)).astype(np.float32) for k in PPO_KEYS}


class Rollout:
    """Host data of one storage of n envs; ``fill(storage)`` records the same data into a RolloutStorage (GPU tests)."""

    def __init__(self, n, seed):
        rs = np.random.RandomState(seed)
        self.n = n
        self.stack = rs.randint(1, 256, (n, 4, 42, 42)).astype(np.uint8)
        self.frames = rs.randint(0, 256, (T, n, 42, 42)).astype(np.uint8)
        self.reset = reset_pattern(PATTERN[n], T, n, seed)
        rows = np.concatenate([np.moveaxis(self.stack[:, 1:], 1, 0), self.frames])
        stacks, depth = rollout_stack_reference(rows, self.reset)
        self.stacks, self.depth = stacks.reshape(T * n, 4, 42, 42), depth.reshape(-1)
        self.unmasked = np.stack([rows[j:j + T] for j in range(4)], axis=2).reshape(T * n, 4, 42, 42)  # fault (c): no plane masked
        self.actions = rs.randint(0, 3, (T, n)).astype(np.int32)
        zero = np.zeros(T * n, np.float32)
        fwd = ppo_loss_reference(base_weights(), self.stacks, self.actions.reshape(-1), zero, zero, zero, HYPER)
        self.logp, self.values = fwd["logp"].astype(np.float32).reshape(T, n), fwd["v"].astype(np.float32).reshape(T, n)
        self.rewards = rs.standard_normal((T, n)).astype(np.float32)
        self.dones = rs.random_sample((T, n)) < 0.2
        self.last = rs.standard_normal(n).astype(np.float32)
        adv, ret = gae_reference(self.rewards, self.values, self.dones, self.last, 0.99, 0.95)
        self.ret = ret.reshape(-1)
        x = adv.reshape(-1).astype(np.float64)
        mean = math.fsum(x) / x.size
        std = math.sqrt(math.fsum((x - mean) ** 2) / (x.size - 1))
        self.adv = ((adv.reshape(-1) - np.float32(mean)) / (np.float32(std) + np.float32(1e-5))).astype(np.float32)  # the gather's rule

    def fill(self, storage):
        storage.begin(torch.from_numpy(self.stack).cuda())
        for t in range(T):
            storage.record(torch.from_numpy(self.frames[t][:, None]).cuda(), torch.from_numpy(self.reset[t]).cuda(), torch.from_numpy(self.values[t]).cuda(),
                           torch.from_numpy(self.actions[t]).cuda(), torch.from_numpy(self.logp[t]).cuda())
            storage.outcome(torch.from_numpy(self.rewards[t]).cuda(), torch.from_numpy(self.dones[t]).cuda())
        storage.finish(torch.from_numpy(self.last).cuda())

    def reference(self, weights, idx, dtype=torch.float64, hyper=HYPER, stacks=None, adv=None):
        return ppo_loss_reference(weights, (self.stacks if stacks is None else stacks)[idx], self.actions.reshape(-1)[idx], self.logp.reshape(-1)[idx],
                                  self.ret[idx], (self.adv if adv is None else adv)[idx], hyper, dtype)


_rollouts = {}


def rollout(n):
    if n not in _rollouts:
        _rollouts[n] = Rollout(n, 300 + n)
    return _rollouts[n]


def rel_err(got, want, keys=PPO_KEYS):
    """per tensor: max|got - want| / max|want| (0 where the tensor's float64 gradient is exactly zero and so is the other)"""
    out = {}
    for k in keys:
        top = float(np.abs(want[k]).max())
        out[k] = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()) / top if top > 0 else float(np.abs(got[k]).max())
    return out


def references32(ro, weights, idx, **kw):
    """the two float32 references on idx: as given, and with the samples in reverse order (per-sample arrays turned back)"""
    fwd = ro.reference(weights, idx, torch.float32, **kw)
    rev = ro.reference(weights, idx[::-1].copy(), torch.float32, **kw)
    for k in ("z1", "z2", "ratio", "logp", "v", "logits", "active"):
        rev[k] = rev[k][::-1]
    return fwd, rev


def seq32(reference, idx, keys=PPO_KEYS, cache=True):
    """The third float32 reference of BIG_CASES, strictly sequential over the samples: the float32 autograd gradient of each sample's own
    loss term (``reference(idx[i:i + 1])``, a batch of one) added one sample at a time, in idx order, into a float32 accumulator and
    divided by float32(B) at the end; the five statistics the same way from the per-sample float32 terms.  ``cache``: a sample that idx
    repeats is evaluated once (the same bits either way; the full-size module turns it off, 4 MB of gradient per sample)."""
    per, acc, stats = {}, None, {k: np.float32(0) for k in STAT_KEYS}
    for p, i in enumerate(idx.tolist()):
        one = per.get(i)
        if one is None:
            r = reference(idx[p:p + 1])
            one = ({k: r["grads"][k] for k in keys}, {k: np.float32(r[k]) for k in STAT_KEYS})
            assert all(g.dtype == np.float32 for g in one[0].values())
            if cache:
                per[i] = one
        acc = {k: one[0][k].copy() for k in keys} if acc is None else {k: acc[k] + one[0][k] for k in keys}
        stats = {k: np.float32(stats[k] + one[1][k]) for k in STAT_KEYS}
    count = np.float32(len(idx))
    assert all(acc[k].dtype == np.float32 for k in keys)
    return dict(grads={k: acc[k] / count for k in keys}, **{k: float(np.float32(stats[k] / count)) for k in STAT_KEYS})


def set_budgets(bt, refs, keys):
    """The budget rule of the module docstring on ``bt.r64`` and the float32 references ``refs`` (two, or three with seq32 last): sets
    errs, e_ref and budget per tensor, stat_errs, stat_e_ref and stat_budget per statistic"""
    bt.ref_names = ("forward", "reverse", "seq32")[:len(refs)]
    bt.errs = [rel_err(r["grads"], bt.r64["grads"], keys) for r in refs]
    bt.e_ref = {k: max(e[k] for e in bt.errs) for k in keys}
    bt.budget = {k: max(FACTOR * bt.e_ref[k], 2 * ULP1) for k in keys}
    # the statistics: absolute errors, FACTOR x e_ref, the floors of the module docstring
    bt.stat_errs = [{k: abs(r[k] - bt.r64[k]) for k in STAT_KEYS} for r in refs]
    bt.stat_e_ref = {k: max(e[k] for e in bt.stat_errs) for k in STAT_KEYS}
    logit_floor = 2 * C.ulp32(np.abs(bt.r64["logits"]).max())
    floor = {k: logit_floor if k in ("policy", "entropy", "kl") else 2 * ULP1 * max(abs(bt.r64[k]), 1.0) for k in STAT_KEYS}
    bt.stat_budget = {k: max(FACTOR * bt.stat_e_ref[k], floor[k]) for k in STAT_KEYS}


class Batch:
    """The kept batch of (n, b) at the learner weights `weights`: idx, the float64 reference, e_ref and the budget per tensor.
    ``sequential``: seq32 joins the two float32 references behind e_ref (BIG_CASES); the screening is the same either way."""

    def __init__(self, n, b, weights, sequential=False):
        self.n, self.b, self.ro = n, b, rollout(n)
        ro, c = self.ro, np.float32(HYPER["clip"])
        rs = np.random.RandomState(1000 * n + b)
        cand = rs.randint(0, T * n, b + b // 4 + 3)
        r64 = ro.reference(weights, cand)
        dz = dr = 0.0
        for r32 in references32(ro, weights, cand):
            dz = max(dz, max(float(np.abs(r32[k] - r64[k]).max()) for k in ("z1", "z2")))
            dr = max(dr, float(np.abs(r32["ratio"] - r64["ratio"]).max()))
        self.delta_z, self.delta_r = 4 * dz, 4 * dr
        zmin = np.minimum(np.abs(r64["z1"]).reshape(len(cand), -1).min(1), np.abs(r64["z2"]).reshape(len(cand), -1).min(1))
        redge = np.minimum(np.abs(r64["ratio"] - (1 - float(c))), np.abs(r64["ratio"] - (1 + float(c))))
        keep = (zmin >= self.delta_z) & (redge >= self.delta_r)
        self.candidates, self.dropped, self.kept = len(cand), int((~keep).sum()), int(keep.sum())
        assert self.kept >= b, (n, b, self.kept)  # every batch fills
        self.idx = cand[keep][:b].copy()
        self.r64 = ro.reference(weights, self.idx)
        refs = references32(ro, weights, self.idx)
        if sequential:
            refs += (seq32(lambda one: ro.reference(weights, one, torch.float32), self.idx),)
        set_budgets(self, refs, PPO_KEYS)

    # ---- fault models: the gradient a subtly wrong kernel would return, in float64
    def fault(self, name, weights):
        g64 = self.r64["grads"]
        if name == "dropped_last":  # the last sample of a partial group never added (the sum is still divided by B)
            if self.b % 8 == 0:
                return None
            if self.b == 1:
                return {k: np.zeros_like(g64[k]) for k in PPO_KEYS}
            part = self.ro.reference(weights, self.idx[:-1])["grads"]
            return {k: part[k] * ((self.b - 1) / self.b) for k in PPO_KEYS}
        if name == "missing_tap":  # conv1's tap (ky, kx) = (3, 3) never accumulated
            g = {k: g64[k].copy() for k in PPO_KEYS}
            g["conv1_w"][:, :, 3, 3] = 0
            return g
        if name == "unmasked":  # every plane read as live
            if (self.ro.depth[self.idx] == 4).all():
                return None
            return self.ro.reference(weights, self.idx, stacks=self.ro.unmasked)["grads"]
        if name == "no_entropy":
            return self.ro.reference(weights, self.idx, hyper=dict(HYPER, ent_coef=0.0))["grads"]
        # ---- between the passes of one workgroup (BIG_CASES): workgroup w of WORKGROUPS takes the groups w, w + WORKGROUPS, ...
        span = GROUP * WORKGROUPS
        if name == "pass_repeats":  # a later pass sees its workgroup's previous inputs: the samples `span` places earlier
            if self.b <= span:
                return None
            idx = self.idx.copy()
            idx[span:] = self.idx[:self.b - span]
            return self.ro.reference(weights, idx)["grads"]
        if name == "earlier_pass_lost":  # a later pass overwrites: only each workgroup's last pass is left (the sum is still divided by B)
            lost = GROUP * max(0, -(-self.b // GROUP) - WORKGROUPS)
            if lost == 0:
                return None
            part = self.ro.reference(weights, self.idx[lost:])["grads"]
            return {k: part[k] * ((self.b - lost) / self.b) for k in PPO_KEYS}
        raise KeyError(name)

    def fault_margin(self, name, weights):
        """the largest (fault's error / budget) over the tensors, or None where the batch cannot show the fault"""
        g = self.fault(name, weights)
        if g is None:
            return None
        e = rel_err(g, self.r64["grads"])
        return max(e[k] / self.budget[k] for k in PPO_KEYS)


FAULTS = ("dropped_last", "missing_tap", "unmasked", "no_entropy")
BIG_FAULTS = FAULTS + ("pass_repeats", "earlier_pass_lost")
_state = {}


def shares(batches):
    act = np.concatenate([b.r64["active"] for b in batches])
    actions = np.concatenate([b.ro.actions.reshape(-1)[b.idx] for b in batches])
    return float((~act).mean()), float(act.mean()), set(actions.tolist())


def chosen():
    """(AMOUNT, the learner's weights, {(n, b): Batch}) -- computed once per process, read-only"""
    if not _state:
        base = base_weights()
        for amount in AMOUNTS:
            w = perturbed(base, amount)
            batches = {(n, b): Batch(n, b, w) for n, b in CASES}
            zero, other, acts = shares(list(batches.values()))
            if zero >= 0.10 and other >= 0.30 and acts == {0, 1, 2}:
                _state.update(amount=amount, weights=w, batches=batches)
                break
        else:
            raise AssertionError("no AMOUNT gives the required shares")
    return _state["amount"], _state["weights"], _state["batches"]


def big():
    """{(n, b): Batch} of BIG_CASES at the weights chosen() chose (they take no part in that choice) -- once per process, read-only"""
    if "big" not in _state:
        w = chosen()[1]
        _state["big"] = {(n, b): Batch(n, b, w, sequential=True) for n, b in BIG_CASES}
    return _state["big"]

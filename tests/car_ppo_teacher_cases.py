"""Teacher data, modes, budgets and fault models shared by tests/test_car_ppo_teacher_rules.py (CPU) and
tests/test_hip_car_ppo_teacher.py (GPU): the device's CarRacing PPO gradient with teacher targets (include/crl.h "car ppo update,
teacher targets") against float64 autograd of the written rule (rules.car_ppo_teacher_loss_reference).  Everything here is computed
from references alone, never from device output.

POOL, WEIGHTS, BATCHES, SCREENING: those of tests/car_ppo_cases.py, unchanged -- ``pool()``, ``chosen()``, ``dead()``, ``big_tail()``.
The teacher term is smooth in the mean and in log_std and adds one branch only, the finiteness of the target, which is a property of
the data, so the screening of the pre-activations and of the ratio's clip edges is all a kept batch needs.

TEACHER DATA per pool sample: ``target`` = the mean of ``rules.car_mlp_reference`` at a second weight draw
(``car_policy_cases.random_weights(2, 2.0)``) on the pool's observations, clamped to [-1, 1] for the point modes (what a driver's
action is); every 11th sample is UNTAUGHT, alternately by a NaN in component 0 and by +inf in component 1 (11 and the pool's
DEAD_EVERY = 17 are coprime: dead and untaught coincide every 187th sample only); ``value_targets`` a seeded normal draw;
``teacher_log_std`` the second draw's ``log_std``; coef = 0.7.

MODES: (CE, point), (CE, Gaussian), (MSE, point), each with policy_term 0 and 1, and (CE, Gaussian, policy_term 1) with value targets.

BUDGET, the rule and FACTOR of car_ppo_cases.Batch: per tensor err = max|g - g64| / max|g64|, e_ref the larger err of the float32
references (forward, reversed; on BIG_TAIL also seq32), budget = max(FACTOR x e_ref, 2 float32 ulps of 1).  STATISTICS: absolute
errors, FACTOR x e_ref with that file's floors; ``term``, ``kl_teacher`` and ``abs_err`` take the floor of ``policy`` (2 float32 ulps
of the batch's largest |log-prob| or |mean|: they are functions of the mean, which is formed from float32 hidden units); ``taught``
is a ratio of two counts and must be exact.

FAULT MODELS (float64): the gradient a subtly wrong teacher kernel would return; test_car_ppo_teacher_rules.py asserts each at least
2 x the budget away on every batch that can show it.
"""
import numpy as np
import torch

from competitive_rl_amd import rules as R
from tests import car_policy_cases as CP
from tests import car_ppo_cases as Q

F = np.float32
KEYS = Q.KEYS
COEF = 0.7
UNTAUGHT_EVERY = 11
T_STAT_KEYS = ("term", "kl_teacher", "abs_err")
STAT_KEYS = Q.STAT_KEYS + T_STAT_KEYS
# name -> (loss, a Gaussian teacher, policy_term, value targets)
MODES = {"ce-point-0": ("ce", False, 0, False), "ce-point-1": ("ce", False, 1, False), "ce-gauss-0": ("ce", True, 0, False),
         "ce-gauss-1": ("ce", True, 1, False), "mse-point-0": ("mse", False, 0, False), "mse-point-1": ("mse", False, 1, False),
         "ce-gauss-1-values": ("ce", True, 1, True)}

_state = {}


class TeacherData:
    def __init__(self, seed=31):
        po = Q.pool()
        self.weights = CP.random_weights(2, 2.0)
        mean, _ = R.car_mlp_reference(self.weights, po.obs)
        assert np.isfinite(mean).all()
        k = np.nonzero(np.arange(po.size) % UNTAUGHT_EVERY == UNTAUGHT_EVERY - 1)[0]
        self.untaught = np.zeros(po.size, bool)
        self.untaught[k] = True

        def marked(t):
            t = t.astype(F).copy()
            t[k[0::2], 0] = np.nan
            t[k[1::2], 1] = np.inf
            return t

        self.target_gauss, self.target_point = marked(mean), marked(np.clip(mean, -1, 1))
        self.value_targets = np.random.RandomState(seed).standard_normal(po.size).astype(F)
        self.log_std = self.weights["log_std"].astype(F)

    def target(self, mode):
        return self.target_gauss if MODES[mode][1] else self.target_point

    def rows(self, mode, idx, **over):
        """the per-sample teacher dict of rules.car_ppo_teacher_loss_reference for the samples ``idx``"""
        loss, gauss, pterm, values = MODES[mode]
        d = dict(target=self.target(mode)[idx], log_std=self.log_std if gauss else None, loss=loss, coef=COEF, policy_term=pterm,
                 value_targets=self.value_targets[idx] if values else None)
        d.update(over)
        return d


def data():
    if "data" not in _state:
        _state["data"] = TeacherData()
    return _state["data"]


def reference(weights, idx, mode, dtype=torch.float64, hyper=Q.HYPER, live=None, **over):
    po = Q.pool()
    lv = po.live if live is None else live
    return R.car_ppo_teacher_loss_reference(weights, po.obs[idx], po.u[idx], po.logp[idx], po.ret[idx], po.adv[idx], lv[idx], hyper, dtype,
                                            teacher=data().rows(mode, idx, **over))


def references32(weights, idx, mode):
    return reference(weights, idx, mode, torch.float32), reference(weights, idx[::-1].copy(), mode, torch.float32)


def seq32(weights, idx, mode):
    """car_ppo_cases.seq32 with the teacher term: each live sample's own float32 gradient (a batch of one) added in idx order into a
    float32 accumulator and divided by float32(max(L, 1)); the teacher statistics summed over the taught samples and divided by
    float32(max(Lt, 1))"""
    po = Q.pool()
    per, acc, L, Lt = {}, {k: np.zeros(R.CAR_POLICY_SHAPES[k], F) for k in KEYS}, 0, 0
    stats = {k: F(0) for k in STAT_KEYS}
    for p, i in enumerate(idx.tolist()):
        if not po.live[i]:
            continue
        one = per.get(i)
        if one is None:
            r = reference(weights, idx[p:p + 1], mode, torch.float32)
            one = per[i] = ({k: r["grads"][k].astype(F) for k in KEYS}, {k: F(r[k]) for k in STAT_KEYS}, bool(r["is_taught"][0]))
        for k in KEYS:
            acc[k] += one[0][k]
        for k in Q.STAT_KEYS:
            stats[k] = F(stats[k] + one[1][k])
        if one[2]:
            for k in T_STAT_KEYS:
                stats[k] = F(stats[k] + one[1][k])
            Lt += 1
        L += 1
    count, tcount = F(max(L, 1)), F(max(Lt, 1))
    out = {k: float(F(stats[k] / (tcount if k in T_STAT_KEYS else count))) for k in STAT_KEYS}
    return dict(grads={k: acc[k] / count for k in KEYS}, taught=Lt / max(L, 1), **out)


class TBatch:
    """A kept batch of car_ppo_cases under one mode: the float64 reference, e_ref and the budgets per tensor and statistic."""

    def __init__(self, base, mode, weights):
        self.base, self.mode, self.idx, self.b = base, mode, base.idx, base.b
        self.live, self.L = base.live, base.L
        self.r64 = reference(weights, self.idx, mode)
        self.taught = self.r64["is_taught"].astype(bool)
        self.Lt = int(self.taught.sum())
        refs = references32(weights, self.idx, mode)
        if len(base.ref_names) == 3:
            refs += (seq32(weights, self.idx, mode),)
        self.errs = [Q.rel_err(r["grads"], self.r64["grads"]) for r in refs]
        self.e_ref = {k: max(e[k] for e in self.errs) for k in KEYS}
        self.budget = {k: max(Q.FACTOR * self.e_ref[k], 2 * Q.ULP1) for k in KEYS}
        assert all(r["taught"] == self.r64["taught"] for r in refs)
        self.stat_e_ref = {k: max(abs(r[k] - self.r64[k]) for r in refs) for k in STAT_KEYS}
        top = max(1.0, float(np.abs(self.r64["logp"][self.live]).max(initial=0)), float(np.abs(self.r64["mean"][self.live]).max(initial=0)))
        logp_floor = 2 * float(np.spacing(F(top)))
        floor = {k: logp_floor if k in ("policy", "kl") + T_STAT_KEYS else 2 * Q.ULP1 * max(abs(self.r64[k]), 1.0) for k in STAT_KEYS}
        self.stat_budget = {k: max(Q.FACTOR * self.stat_e_ref[k], floor[k]) for k in STAT_KEYS}

    # ---- fault models: the gradient a subtly wrong teacher kernel would return, in float64
    def fault(self, name, weights):
        loss, gauss, pterm, values = MODES[self.mode]
        g64, L, Lt, idx, d = self.r64["grads"], self.L, self.Lt, self.idx, data()
        po = Q.pool()
        if L == 0:
            return None
        tgt = d.target(self.mode)
        only_teacher = dict(hyper=dict(Q.HYPER, vf_coef=0.0, ent_coef=0.0), policy_term=0)  # the loss is coef * term alone
        if name == "target_row_b":  # the target of row b instead of row idx[b]
            rows = np.arange(len(idx)) % po.size
            if not (self.live & (idx != rows)).any():
                return None
            over = dict(target=tgt[rows])
            if values:
                over["value_targets"] = d.value_targets[rows]
            return reference(weights, idx, self.mode, **over)["grads"]
        if name == "teacher_on_dead":  # a dead sample's teacher term added (the sum is still divided by L)
            dead_taught = ~self.live & np.isfinite(tgt[idx]).all(1)
            if not dead_taught.any():
                return None
            lv = np.zeros(po.size, bool)
            lv[idx[dead_taught]] = True
            keep = np.nonzero(dead_taught)[0]
            extra = reference(weights, idx[keep], self.mode, live=lv, **only_teacher)
            return {k: g64[k] + extra["grads"][k] * (len(keep) / L) for k in KEYS}
        if name == "untaught_as_zero_target":  # a non-finite target float read as 0 and the sample taught
            if not (self.live & ~self.taught).any():
                return None
            return reference(weights, idx, self.mode, target=np.where(np.isfinite(tgt[idx]), tgt[idx], F(0)))["grads"]
        if name == "mean_over_taught":  # the teacher term divided by Lt, the rest by L
            if Lt == 0 or Lt == L:
                return None
            plain = reference(weights, idx, self.mode, coef=0.0)["grads"]
            return {k: plain[k] + (g64[k] - plain[k]) * (L / Lt) for k in KEYS}
        if name == "no_logstd_term":  # CE: t_ls missing from log_std's gradient
            if loss != "ce" or Lt == 0:
                return None
            g = {k: g64[k].copy() for k in KEYS}
            g["log_std"] = reference(weights, idx, self.mode, coef=0.0)["grads"]["log_std"]
            return g
        if name == "sq_dropped":  # a Gaussian teacher's spread taken as 0
            if not gauss or Lt == 0:
                return None
            return reference(weights, idx, self.mode, log_std=None)["grads"]
        if name == "policy_term_ignored":  # policy_term = 0 treated as 1
            if pterm == 1 or not self.r64["active"][self.live].any():
                return None
            return reference(weights, idx, self.mode, policy_term=1)["grads"]
        if name == "value_targets_ignored":
            return reference(weights, idx, self.mode, value_targets=None)["grads"] if values else None
        if name == "coef_ignored":  # coef taken as 1
            return None if Lt == 0 else reference(weights, idx, self.mode, coef=1.0)["grads"]
        raise KeyError(name)

    def fault_margin(self, name, weights):
        """the largest (fault's error / budget) over the tensors, or None where the batch cannot show the fault"""
        g = self.fault(name, weights)
        if g is None:
            return None
        e = Q.rel_err(g, self.r64["grads"])
        return max(e[k] / self.budget[k] for k in KEYS)


FAULTS = ("target_row_b", "teacher_on_dead", "untaught_as_zero_target", "mean_over_taught", "no_logstd_term", "sq_dropped",
          "policy_term_ignored", "value_targets_ignored", "coef_ignored")
WHICH = tuple(Q.CASES) + ("dead", "big_tail")


def base_of(which):
    return {"big_tail": Q.big_tail, "dead": Q.dead}[which]() if isinstance(which, str) else Q.chosen()[2][which]


def batch(which, mode):
    """the TBatch of one of WHICH under ``mode`` at the weights chosen() chose -- once per process, read-only"""
    key = (which, mode)
    if key not in _state:
        _state[key] = TBatch(base_of(which), mode, Q.chosen()[1])
    return _state[key]

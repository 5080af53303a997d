"""Pools, batches, the error budget and the fault models shared by tests/test_car_ppo_rules.py (CPU) and tests/test_hip_car_ppo.py (GPU):
the device's CarRacing PPO gradient (include/crl.h "car ppo update") against float64 autograd of the written rule
(rules.car_ppo_loss_reference).  Everything here is computed from references alone, never from device output.

POOL.  T = 6 steps of N = 24 envs x 2 cars = 288 samples, as a CarRolloutStorage of cars (0, 1) holds them.  The observations are those
of the CPU checker's 8 seeded tracks, both cars, at 18 moments of a RULE_BASED drive with epsilon 0.3; every 17th sample is DEAD (an
all-zero observation, action, value and log-prob 0, live = 0), as the device stores a done car.  Actions, log-probs and values are
``rules.car_policy_reference`` of the UNPERTURBED weights ``car_policy_cases.random_weights(1, 2.0)``; rewards are normal, 20 % dones;
returns and advantages by ``rules.gae_reference``, normalised over the live samples by the storage's rule.  The learner holds the
weights perturbed by AMOUNT x each tensor's standard deviation x a seeded normal draw -- the AMOUNT rule of tests/ppo_cases.py: the
first of its AMOUNTS at which, over the kept live samples of all batches of CASES, at least 10 % lie in the zero-gradient branch of the
clipped ratio and at least 30 % in the other.

BATCHES.  B in CASES = {1, 7, G, G + 1, 130} with G = 64, the samples of a group (csrc/car_ppo.hip), and BIG = G * W + G + 1 = 65 601
with W = 1024, the most workgroups: the smallest B at which a workgroup (workgroup 0) takes a second group while the last group is
partial (one sample).  ``idx`` is drawn with replacement (shuffled, duplicates).  DEAD_CASE: 9 entries, all dead (L = 0).
BIG_TAIL: BIG entries of which the first BIG - 1 are dead and the last -- the one sample of the partial last group, which workgroup 0
takes as its SECOND group -- is the live sample of the batch of 1: L = 1, so that sample IS the gradient.  One sample among the
61 907 live ones of BIG changes the mean by 1.6e-5 of itself, below any float32 budget at that size (``dropped_last`` is not
claimed there); on BIG_TAIL a kernel that loses the last group's sample returns zeros.

SCREENING, the rule of tests/ppo_cases.py: a live candidate is dropped if a pre-activation lies within dz of 0 or r within dr of
1 +- c; dz and dr are each 4 x the largest deviation of the two float32 references (forward and reversed order) from float64 on the
candidates.  At most 10 % of all candidates may be dropped (test_car_ppo_rules.py asserts it).

BUDGET, the rule and FACTOR of tests/ppo_cases.py: per tensor err = max|g - g64| / max|g64|, e_ref the larger err of the float32
references, budget = max(FACTOR x e_ref, 2 float32 ulps of 1).  BIG uses three float32 references: forward, reverse and seq32, the
strictly sequential float32 sum of the per-sample gradients in idx order divided by float32(max(L, 1)).
STATISTICS: absolute errors, FACTOR x e_ref, with the floors of ppo_cases.py: for the policy loss and the approximate KL 2 float32
ulps of the batch's largest |log-prob| or |mean| (they are functions of a log-probability formed from float32 hidden units, which
cannot be known better than its mean), and 2 ulps of max(|statistic|, 1) for the value loss, the entropy and the clipped share.

FAULT MODELS (float64): the gradient a subtly wrong kernel would return; test_car_ppo_rules.py asserts each at least 2 x the budget
away on every batch that can show it.  ent_coef of the test is 0.01, chosen for that: the missing ``- ent`` changes log_std's gradient
by 0.01 against a budget near 1e-5 of its largest entry.
"""
import math

import numpy as np
import torch

from competitive_rl_amd import rules as R
from tests import car_policy_cases as CP
from tests import ppo_cases as P

F = np.float32
KEYS = R.CAR_POLICY_KEYS
STAT_KEYS = R.CAR_PPO_STAT_KEYS
T, N_ENVS, CARS = 6, 24, 2
ROWS = N_ENVS * CARS
GROUP, WORKGROUPS = 64, 1024  # csrc/car_ppo.hip: samples per group, the most workgroups a launch has
FACTOR = P.FACTOR
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
CASES = (1, 7, GROUP, GROUP + 1, 130)
BIG = GROUP * WORKGROUPS + GROUP + 1
DEAD_CASE = 9
AMOUNTS = P.AMOUNTS
ULP1 = 2.0 ** -23
DEAD_EVERY = 17


def base_weights():
    return CP.random_weights(1, 2.0)


def perturbed(base, amount, seed=5):
    rs = np.random.RandomState(seed)
    return {k: (base[k] + F(amount) * F(base[k].std()) * rs.standard_normal(base[k].shape).astype(F)).astype(F) for k in KEYS}


def checker_observations(count):
    """``count`` observations [count, 21] of both cars of the checker's 8 tracks along a RULE_BASED drive with epsilon 0.3"""
    B, boxes, n = CP.checker_tracks(8)
    style = R.check_car_style(epsilon=0.3)
    out, t = [], 0
    while sum(len(o) for o in out) < count:
        for _ in range(5):
            acts = np.zeros((8, 2, 2), F)
            for c in range(2):
                hull, wheels = CP._driver_inputs(B.E, c)
                acts[:, c] = R.car_driver_reference(hull, wheels, B.E["done"][:, c], boxes, n, style, 1, np.arange(8), c, t)
            B.step(acts.astype(np.float64))
            t += 1
        out += [CP.obs_of_batch(B.E, c, boxes, n) for c in range(2)]
    return np.concatenate(out)[:count].astype(F)


class Pool:
    """Host data of one finished CarRolloutStorage of T steps, N_ENVS envs and both cars; ``fill(storage)`` loads it (GPU tests)."""

    def __init__(self, seed=77):
        rs = np.random.RandomState(seed)
        S = T * ROWS
        self.size = S
        self.live = (np.arange(S) % DEAD_EVERY != DEAD_EVERY - 1)
        self.obs = checker_observations(S)
        self.obs[~self.live] = 0
        fwd = R.car_policy_reference(base_weights(), self.obs, self.live, False, seed=9, gid=np.arange(S) % N_ENVS, car=0, call=np.arange(S) // ROWS)
        self.u, self.logp, self.values = fwd["u"], fwd["log_prob"], fwd["value"]
        self.rewards = rs.standard_normal((T, ROWS)).astype(F)
        self.dones = rs.random_sample((T, ROWS)) < 0.2
        self.last = rs.standard_normal(ROWS).astype(F)
        adv, ret = R.gae_reference(self.rewards, self.values.reshape(T, ROWS), self.dones, self.last, 0.99, 0.95)
        self.raw_adv, self.ret = adv.reshape(-1), ret.reshape(-1)
        x = self.raw_adv[self.live].astype(np.float64)
        self.mean = math.fsum(x) / x.size
        self.std = math.sqrt(math.fsum((x - self.mean) ** 2) / (x.size - 1))
        self.adv = ((self.raw_adv - F(self.mean)) / (F(self.std) + F(1e-5))).astype(F)  # the gather's rule

    def lines(self):
        """the storage's sample lines, uint32 [T * ROWS, 32] (include/crl.h "car rollout storage")"""
        ln = np.zeros((self.size, 32), F)
        ln[:, :21], ln[:, 21:23], ln[:, 23], ln[:, 24] = self.obs, self.u, self.logp, self.values
        ln[:, 25], ln[:, 26], ln[:, 27] = self.rewards.reshape(-1), self.ret, self.raw_adv
        out = ln.view(np.uint32)
        out[:, 28] = self.live.astype(np.uint32) | (self.dones.reshape(-1).astype(np.uint32) << 1)
        return out

    def fill(self, storage):
        storage.load_state_dict({"kind": "CarRolloutStorage", "num_steps": T, "num_envs": N_ENVS, "players": 2, "cars": (0, 1), "gamma": 0.99,
                                 "gae_lambda": 0.95, "normalize_advantage": True, "state": "finished", "step": T, "outcomes": T,
                                 "contents": {"lines": self.lines(), "stats": np.array([self.mean, self.std, float(self.live.sum())]), "normalized": True}})

    def reference(self, weights, idx, dtype=torch.float64, hyper=HYPER, live=None):
        lv = self.live if live is None else live
        return R.car_ppo_loss_reference(weights, self.obs[idx], self.u[idx], self.logp[idx], self.ret[idx], self.adv[idx], lv[idx], hyper, dtype)


_state = {}


def pool():
    if "pool" not in _state:
        _state["pool"] = Pool()
    return _state["pool"]


def rel_err(got, want):
    """per tensor: max|got - want| / max|want| (the largest |got| where the float64 gradient is exactly zero)"""
    out = {}
    for k in KEYS:
        top = float(np.abs(want[k]).max())
        out[k] = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()) / top if top > 0 else float(np.abs(got[k]).max())
    return out


def references32(po, weights, idx):
    fwd = po.reference(weights, idx, torch.float32)
    rev = po.reference(weights, idx[::-1].copy(), torch.float32)
    for k in ("a", "ratio", "logp", "v", "mean", "active"):
        rev[k] = rev[k][::-1]
    return fwd, rev


def seq32(po, weights, idx):
    """The third float32 reference: the float32 autograd gradient of each live sample's own loss term (a batch of one) added one
    sample at a time, in idx order, into a float32 accumulator and divided by float32(max(L, 1)); the statistics the same way."""
    per, acc, stats, L = {}, {k: np.zeros(R.CAR_POLICY_SHAPES[k], F) for k in KEYS}, {k: F(0) for k in STAT_KEYS}, 0
    for p, i in enumerate(idx.tolist()):
        if not po.live[i]:
            continue
        one = per.get(i)
        if one is None:
            r = po.reference(weights, idx[p:p + 1], torch.float32)
            one = per[i] = ({k: r["grads"][k].astype(F) for k in KEYS}, {k: F(r[k]) for k in STAT_KEYS})
        for k in KEYS:
            acc[k] += one[0][k]
        stats = {k: F(stats[k] + one[1][k]) for k in STAT_KEYS}
        L += 1
    count = F(max(L, 1))
    return dict(grads={k: acc[k] / count for k in KEYS}, **{k: float(F(stats[k] / count)) for k in STAT_KEYS})


class Batch:
    """The kept batch of ``b`` samples at the learner weights: idx, the float64 reference, e_ref and the budget per tensor."""

    def __init__(self, b, weights, sequential=False, dead_only=False, idx=None):
        po = self.po = pool()
        self.b, c = b, float(F(HYPER["clip"]))
        rs = np.random.RandomState(1000 + b)
        if idx is not None:  # (entries screened by the batches they come from)
            cand = np.asarray(idx)
            assert len(cand) == b
        elif dead_only:
            cand = rs.choice(np.nonzero(~po.live)[0], b)
        else:
            cand = rs.randint(0, po.size, b + b // 4 + 3)
        r64 = po.reference(weights, cand)
        dz = dr = 0.0
        for r32 in references32(po, weights, cand):
            dz = max(dz, float(np.abs(r32["a"] - r64["a"]).max()))
            dr = max(dr, float(np.abs(r32["ratio"] - r64["ratio"]).max()))
        self.delta_z, self.delta_r = 4 * dz, 4 * dr
        lv = po.live[cand]
        zmin = np.abs(r64["a"]).min(1)
        redge = np.minimum(np.abs(r64["ratio"] - (1 - c)), np.abs(r64["ratio"] - (1 + c)))
        keep = ~lv | ((zmin >= self.delta_z) & (redge >= self.delta_r))
        self.candidates, self.dropped, self.kept = len(cand), int((~keep).sum()), int(keep.sum())
        assert self.kept >= b, (b, self.kept)  # every batch fills
        self.idx = cand[keep][:b].copy()
        self.r64 = po.reference(weights, self.idx)
        self.live = po.live[self.idx]
        self.L = int(self.live.sum())
        refs = references32(po, weights, self.idx)
        if sequential:
            refs += (seq32(po, weights, self.idx),)
        self.ref_names = ("forward", "reverse", "seq32")[:len(refs)]
        self.errs = [rel_err(r["grads"], self.r64["grads"]) for r in refs]
        self.e_ref = {k: max(e[k] for e in self.errs) for k in KEYS}
        self.budget = {k: max(FACTOR * self.e_ref[k], 2 * ULP1) for k in KEYS}
        self.stat_errs = [{k: abs(r[k] - self.r64[k]) for k in STAT_KEYS} for r in refs]
        self.stat_e_ref = {k: max(e[k] for e in self.stat_errs) for k in STAT_KEYS}
        top = max(1.0, float(np.abs(self.r64["logp"][self.live]).max(initial=0)), float(np.abs(self.r64["mean"][self.live]).max(initial=0)))
        logp_floor = 2 * float(np.spacing(F(top)))
        floor = {k: logp_floor if k in ("policy", "kl") else 2 * ULP1 * max(abs(self.r64[k]), 1.0) for k in STAT_KEYS}
        self.stat_budget = {k: max(FACTOR * self.stat_e_ref[k], floor[k]) for k in STAT_KEYS}

    # ---- fault models: the gradient a subtly wrong kernel would return, in float64
    def fault(self, name, weights):
        po, g64, L, b = self.po, self.r64["grads"], self.L, self.b
        scaled = lambda g, s: {k: g[k] * s for k in KEYS}  # noqa: E731
        if L == 0:
            return None
        if name == "dropped_last":  # the last sample never added (the sum is still divided by L)
            if not self.live[-1] or (b > GROUP * WORKGROUPS and L > 1):  # (BIG: see BIG_TAIL in the module docstring)
                return None
            if L == 1:
                return {k: np.zeros_like(g64[k]) for k in KEYS}
            return scaled(po.reference(weights, self.idx[:-1])["grads"], (L - 1) / L)
        if name == "dead_unmasked":  # a dead sample's terms added (the sum is still divided by L)
            if L == b:
                return None
            return scaled(po.reference(weights, self.idx, live=np.ones(po.size, bool))["grads"], b / L)
        if name == "mean_over_b":  # the mean divided by B instead of L
            return None if L == b else scaled(g64, L / b)
        if name == "no_entropy":  # the - ent of the log_std gradient missing
            return po.reference(weights, self.idx, hyper=dict(HYPER, ent_coef=0.0))["grads"]
        if name == "no_zz_term":  # the zz^2 - 1 term missing: log_std's gradient is - ent alone
            g = {k: g64[k].copy() for k in KEYS}
            g["log_std"][:] = -float(F(HYPER["ent_coef"]))
            return g
        if name == "hidden_unit_dropped":  # hidden unit 64 (the first second unit of a serving lane) takes no part
            w = {k: np.array(weights[k]) for k in KEYS}
            w["policy_w"][:, 64], w["value_w"][:, 64] = 0, 0
            g = po.reference(w, self.idx)["grads"]
            g["policy_w"][:, 64], g["value_w"][:, 64] = 0, 0
            return g
        if name == "feature_20_dropped":
            g = {k: g64[k].copy() for k in KEYS}
            g["fc1_w"][:, 20] = 0
            return g
        if name == "second_pass_overwrites":  # only each workgroup's last group is left (the sum is still divided by L)
            lost = GROUP * max(0, -(-b // GROUP) - WORKGROUPS)
            if lost == 0 or not self.live[:lost].any():  # (nothing live among the overwritten entries: the batch cannot show it)
                return None
            part = po.reference(weights, self.idx[lost:])
            return scaled(part["grads"], part["live"] / L)
        raise KeyError(name)

    def fault_margin(self, name, weights):
        """the largest (fault's error / budget) over the tensors, or None where the batch cannot show the fault"""
        g = self.fault(name, weights)
        if g is None:
            return None
        e = rel_err(g, self.r64["grads"])
        return max(e[k] / self.budget[k] for k in KEYS)


FAULTS = ("dropped_last", "dead_unmasked", "mean_over_b", "no_entropy", "no_zz_term", "hidden_unit_dropped", "feature_20_dropped",
          "second_pass_overwrites")


def shares(batches):
    act = np.concatenate([b.r64["active"][b.live] for b in batches])
    return float((~act).mean()), float(act.mean())


def chosen():
    """(AMOUNT, the learner's weights, {b: Batch}) -- computed once per process, read-only"""
    if "amount" not in _state:
        base = base_weights()
        for amount in AMOUNTS:
            w = perturbed(base, amount)
            batches = {b: Batch(b, w) for b in CASES}
            zero, other = shares(list(batches.values()))
            if zero >= 0.10 and other >= 0.30:
                _state.update(amount=amount, weights=w, batches=batches)
                break
        else:
            raise AssertionError("no AMOUNT gives the required shares")
    return _state["amount"], _state["weights"], _state["batches"]


def big():
    """the Batch of BIG at the weights chosen() chose (it takes no part in that choice) -- once per process, read-only"""
    if "big" not in _state:
        _state["big"] = Batch(BIG, chosen()[1], sequential=True)
    return _state["big"]


def big_tail():
    """BIG_TAIL: BIG - 1 dead entries, then the live sample of the batch of 1"""
    if "big_tail" not in _state:
        _, w, batches = chosen()
        idx = np.concatenate([np.resize(dead().idx, BIG - 1), batches[1].idx])
        _state["big_tail"] = Batch(BIG, w, sequential=True, idx=idx)
    return _state["big_tail"]


def dead():
    """the all-dead Batch (L = 0)"""
    if "dead" not in _state:
        _state["dead"] = Batch(DEAD_CASE, chosen()[1], dead_only=True)
    return _state["dead"]

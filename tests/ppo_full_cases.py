"""Rollouts, batches, the error budget and the fault models shared by tests/test_ppo_full_rules.py (CPU) and tests/test_hip_ppo_full.py
(GPU): the device's full-size PPO gradient (include/crl.h "ppo update, full size") against float64 autograd of the written rule
(rules.ppo_full_loss_reference).  The method, the budget rule and FACTOR = 10 are those of tests/ppo_cases.py (its docstring has the
reasons); everything here is computed from references alone, never from device output.

ROLLOUTS.  As ppo_cases.Rollout: T = 6, N in {1, 11, 67}, the same reset patterns and seeds, uniform byte frames, normalisation on.  The
stored log-probs and values are those of the UNPERTURBED ``policy_full_weights.make_weights(2024)`` (float64 forward, rounded to
float32); the learner holds them perturbed by AMOUNT x each tensor's standard deviation x a seeded normal draw.  AMOUNT is the first
of AMOUNTS = (0.1, 0.2, 0.3, 0.5) with at least 10 % of the kept samples in the zero-gradient branch, at least 30 % in the other and all
three actions (the light list 0.002 .. 0.1 never reaches 10 % on this network: its stored values are of another scale).

BATCHES.  CASES of ppo_cases; ``b + b // 2 + 4`` candidates per batch, screened on z1, z2, z3 and the two clip edges with 4 x the float32
references' deviation as the margin.  The full network has 20 128 pre-activations per sample against 8 000, so more candidates sit
near a kink: at most 20 % of all candidates may be dropped (test_ppo_full_rules.py asserts the cap); every batch must still fill (Batch asserts it).

BUDGET per tensor max(FACTOR x e_ref, 2 ulp), statistics as in ppo_cases.

FAULT MODELS: dropped_last (the batch's last sample never added), missing_tap (conv2's tap (3, 3) never accumulated), unmasked,
no_entropy, w3_last_row (the conv3_w gradient alone lacks the batch's last sample: the K tail of the gW3 product).

BIG_CASES, (N 67, B 601), run at the default scratch_rows and at BIG_ROWS = 320.  With B <= 130 (and 130 rows in chunks of 64) every
workgroup of ppo_full_back_kernel sees at most one row per launch, the two-level head sum has one slice per chunk and the front kernel's
row loop runs once: nothing in CASES holds gW1 / gW2 / gb1 / gb2 across rows while the LDS tiles are re-filled, adds a second slice, or
adds several slices onto a previous chunk's sum -- which production (B 65 536 in chunks of 16 384: 64 rows per workgroup, 64 slices) does
all the time.  601 rows in one chunk: the back kernel's 256 workgroups take three rows (0 .. 88) or two; three head slices 256 + 256 +
89; the front loop runs twice on 89 of 512 workgroups; the last heads workgroup holds one row; 601 % 4 = 1, so dropped_last and
w3_last_row show.  In chunks of 320: 320 and 281 rows, each two slices with a partial second one, W = 256 with one or two rows per
workgroup, the second chunk adding onto the first one's sums.  ``big()`` builds the batch on rollout(67) at the weights chosen() has
chosen, by the same candidate draw and screening (905 candidates, 102 dropped = 11.3 %, its own cap DROP_CAP); it takes no part in
chosen()'s shares, AMOUNT or the cap over CASES, which come out bit-identical.

Its e_ref is over THREE float32 references: forward, reverse and ppo_cases.seq32 (per-sample float32 gradients added one at a time in
idx order, / float32(B)); ppo_cases' docstring has the reason and the measured ratios (critic_b: seq32 is 11 x the two-reference e_ref).

FAULT MODELS between rows, slices and chunks (BIG_FAULTS, float64): pass_repeats -- a later row sees its workgroup's previous inputs:
the samples at positions >= 256 are those 256 places earlier; earlier_pass_lost -- a later row overwrites: only each workgroup's last
row (positions 345 .. 600) is left, the sum still divided by B; slice_lost -- wa, ba, wc, bc and b3 lack the rows of the last slice
(512 .. 600); chunk_restart -- the run at BIG_ROWS: every tensor holds the second chunk's sum alone, divided by B.
"""
import math

import numpy as np
import torch

from competitive_rl_amd.rules import PPO_FULL_KEYS, gae_reference, ppo_full_loss_reference, rollout_stack_reference
from tests.policy_full_weights import make_weights
from tests.ppo_cases import CASES, FACTOR, HYPER, PATTERN, STAT_KEYS, ULP1, T, seq32, set_budgets
from tests.test_rollout_storage_rules import reset_pattern

KEYS = PPO_FULL_KEYS
HEAD_KEYS = ("conv3_b", "actor_w", "actor_b", "critic_w", "critic_b")  # what the two-level head sum forms
AMOUNTS = (0.1, 0.2, 0.3, 0.5)
DROP_CAP = 0.20
PRE = ("z1", "z2", "z3")
BIG_CASES = ((67, 601),)  # (three rows per workgroup, three head slices; in chunks of BIG_ROWS two chunks of two slices: see above)
BIG_ROWS = 320            # scratch_rows of the chunked run of BIG_CASES
SLICE, BACK_MAX = 256, 256  # pong_ppo_full.hip: rows per head slice, the most workgroups the back kernel has


def base_weights():
    return make_weights(2024)


def perturbed(base, amount, seed=5):
    rs = np.random.RandomState(seed)
    return {k: (base[k] + np.float32(amount) * np.float32(base[k].std() if base[k].size > 1 else abs(base[k]).max()) *
                rs.standard_normal(base[k].shape).astype(np.float32)).astype(np.float32) for k in KEYS}


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
        self.unmasked = np.stack([rows[j:j + T] for j in range(4)], axis=2).reshape(T * n, 4, 42, 42)  # fault: no plane masked
        self.actions = rs.randint(0, 3, (T, n)).astype(np.int32)
        zero = np.zeros(T * n, np.float32)
        fwd = ppo_full_loss_reference(base_weights(), self.stacks, self.actions.reshape(-1), zero, zero, zero, HYPER)
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

    def reference(self, weights, idx, dtype=torch.float64, hyper=HYPER, stacks=None):
        return ppo_full_loss_reference(weights, (self.stacks if stacks is None else stacks)[idx], self.actions.reshape(-1)[idx], self.logp.reshape(-1)[idx],
                                       self.ret[idx], self.adv[idx], hyper, dtype)


_rollouts = {}


def rollout(n):
    if n not in _rollouts:
        _rollouts[n] = Rollout(n, 300 + n)
    return _rollouts[n]


def rel_err(got, want):
    """per tensor: max|got - want| / max|want| (0 where the tensor's float64 gradient is exactly zero and so is the other)"""
    out = {}
    for k in KEYS:
        top = float(np.abs(want[k]).max())
        out[k] = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()) / top if top > 0 else float(np.abs(got[k]).max())
    return out


def references32(ro, weights, idx):
    """the two float32 references on idx: as given, and with the samples in reverse order (per-sample arrays turned back)"""
    fwd = ro.reference(weights, idx, torch.float32)
    rev = ro.reference(weights, idx[::-1].copy(), torch.float32)
    for k in PRE + ("ratio", "logp", "v", "logits", "active"):
        rev[k] = rev[k][::-1]
    return fwd, rev


class Batch:
    """The kept batch of (n, b) at the learner weights `weights`: idx, the float64 reference, e_ref and the budget per tensor"""

    def __init__(self, n, b, weights, sequential=False):
        self.n, self.b, self.ro = n, b, rollout(n)
        ro, c = self.ro, np.float32(HYPER["clip"])
        rs = np.random.RandomState(1000 * n + b)
        cand = rs.randint(0, T * n, b + b // 2 + 4)
        r64 = ro.reference(weights, cand)
        dz = dr = 0.0
        for r32 in references32(ro, weights, cand):
            dz = max(dz, max(float(np.abs(r32[k] - r64[k]).max()) for k in PRE))
            dr = max(dr, float(np.abs(r32["ratio"] - r64["ratio"]).max()))
        self.delta_z, self.delta_r = 4 * dz, 4 * dr
        zmin = np.min([np.abs(r64[k]).reshape(len(cand), -1).min(1) for k in PRE], axis=0)
        redge = np.minimum(np.abs(r64["ratio"] - (1 - float(c))), np.abs(r64["ratio"] - (1 + float(c))))
        keep = (zmin >= self.delta_z) & (redge >= self.delta_r)
        self.candidates, self.dropped, self.kept = len(cand), int((~keep).sum()), int(keep.sum())
        assert self.kept >= b, (n, b, self.kept)  # every batch fills
        self.idx = cand[keep][:b].copy()
        self.r64 = ro.reference(weights, self.idx)
        refs = references32(ro, weights, self.idx)
        if sequential:
            refs += (seq32(lambda one: ro.reference(weights, one, torch.float32), self.idx, KEYS, cache=False),)
        set_budgets(self, refs, KEYS)  # (FACTOR x e_ref, the floors of ppo_cases' docstring)

    # ---- fault models: the gradient a subtly wrong kernel would return, in float64
    def _only(self, weights, lo, hi):
        """the samples at positions [lo, hi) alone, the sum still divided by B"""
        if hi <= lo:
            return {k: np.zeros_like(self.r64["grads"][k]) for k in KEYS}
        part = self.ro.reference(weights, self.idx[lo:hi])["grads"]
        return {k: part[k] * ((hi - lo) / self.b) for k in KEYS}

    def _without_last(self, weights):
        return self._only(weights, 0, self.b - 1)

    def fault(self, name, weights):
        g64 = self.r64["grads"]
        if name == "dropped_last":  # the last sample of a partial step of four rows never added (the sum is still divided by B)
            return None if self.b % 4 == 0 else self._without_last(weights)
        if name == "missing_tap":  # conv2's tap (ky, kx) = (3, 3) never accumulated
            g = {k: g64[k].copy() for k in KEYS}
            g["conv2_w"][:, :, 3, 3] = 0
            return g
        if name == "unmasked":  # every plane read as live
            if (self.ro.depth[self.idx] == 4).all():
                return None
            return self.ro.reference(weights, self.idx, stacks=self.ro.unmasked)["grads"]
        if name == "no_entropy":
            return self.ro.reference(weights, self.idx, hyper=dict(HYPER, ent_coef=0.0))["grads"]
        if name == "w3_last_row":  # the K tail of the gW3 product: conv3_w alone lacks the last sample
            return dict(g64, conv3_w=self._without_last(weights)["conv3_w"])
        # ---- between the rows of one workgroup, the slices and the chunks (BIG_CASES)
        if name == "pass_repeats":  # a later row sees its workgroup's previous inputs: the samples BACK_MAX places earlier
            if self.b <= BACK_MAX:
                return None
            idx = self.idx.copy()
            idx[BACK_MAX:] = self.idx[:self.b - BACK_MAX]
            return self.ro.reference(weights, idx)["grads"]
        if name == "earlier_pass_lost":  # a later row overwrites: only each workgroup's last row is left
            return None if self.b <= BACK_MAX else self._only(weights, self.b - BACK_MAX, self.b)
        if name == "slice_lost":  # the head tensors lack the rows of the last slice
            if self.b <= SLICE:
                return None
            part = self._only(weights, 0, SLICE * ((self.b - 1) // SLICE))
            return dict(g64, **{k: part[k] for k in HEAD_KEYS})
        if name == "chunk_restart":  # the run at BIG_ROWS: every tensor holds the last chunk's sum alone
            return None if self.b <= BIG_ROWS else self._only(weights, BIG_ROWS * ((self.b - 1) // BIG_ROWS), self.b)
        raise KeyError(name)

    def fault_margin(self, name, weights):
        """the largest (fault's error / budget) over the tensors, or None where the batch cannot show the fault"""
        g = self.fault(name, weights)
        if g is None:
            return None
        e = rel_err(g, self.r64["grads"])
        return max(e[k] / self.budget[k] for k in KEYS)


FAULTS = ("dropped_last", "missing_tap", "unmasked", "no_entropy", "w3_last_row")
BIG_FAULTS = FAULTS + ("pass_repeats", "earlier_pass_lost", "slice_lost", "chunk_restart")
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

"""The critic head's error budget, its fault claims and the small helpers shared by tests/test_rollout_rules.py (CPU) and
tests/test_hip_rollout.py (GPU): the value of crl_policy_act_rollout against a float64 forward pass.

THE VALUE'S BUDGET is the logits' rule of tests/policy_f64_cases.py applied to element [1] of the oracle's forward functions, over
references only (never over device output):
    e_ref  = the largest |r - forward64 value| over the rows of the batch, r over the float32 references: BLAS order
             (policy_oracle.forward / forward_full), strictly sequential order (forward_seq32) and, where the reference's torch module
             recorded a value for the rows (tests/golden), the recording;
    budget = FACTOR * e_ref, and never below 2 float32 ulps of the batch's largest |value|.
The selector and wide weight sets carry their base set's critic (MEDIUM's resp. make_weights(5)'s): their actor is made up, their
features are not.
"""
import os

import numpy as np

from oracle import policy_oracle as P
from tests import policy_f64_cases as C

FACTOR = 2  # the rule allows 2 .. 4 (test_policy_f64_reference.py); docs/LAB_NOTES_rollout.md has the device's measured ratios
GOLD = os.path.join(C.ROOT, "tests", "golden")

# (weight set, input kind) -> the fault models of policy_f64_cases.FAULTS that the VALUE of the batch is relied on to detect: the model's
# error in the value is at least 2 x budget there (measured on the CPU: (b) 5.4 .. 23.8 x budget on the light batches, (b) and (c) 3.0 ..
# 10.2 x on the full-size ones, (a) 3.8 .. 7.6 x where it is claimed).  test_rollout_rules.py asserts every claim.
VALUE_CLAIMS = {**{k: "b" for k in C.LIGHT_CASES}, **{k: "bc" for k in C.FULL_CASES}}
for _k in (("weak", "dense"), ("medium", "dense"), ("light_selector", "sparse"), ("full_selector", "dense"), ("full_selector", "sparse")):
    VALUE_CLAIMS[_k] = "a" + VALUE_CLAIMS[_k]


def value_references(wts, stacks, full, recorded=None):
    """(forward64 values [B], e_ref, {reference name: its largest error}) of one batch of stacks [B, 4, 42, 42]"""
    v64 = P.forward64(wts, stacks, full)[1]
    errs = {"blas32": float(np.abs((P.forward_full if full else P.forward)(wts, stacks)[1] - v64).max()),
            "seq32": float(np.abs(P.forward_seq32(wts, stacks, full)[1] - v64).max())}
    if recorded is not None:
        errs["recorded"] = float(np.abs(np.asarray(recorded, np.float64) - v64).max())
    return v64, max(errs.values()), errs


def value_budget_of(v64, e_ref, factor=FACTOR):
    return max(factor * e_ref, 2 * C.ulp32(np.abs(v64).max()))


_cache = {}


class ValueCase:
    """The value side of policy_f64_cases.case(ws, kind): float64 values [CALLS - WARMUP, UNIQUE] of the compared calls, e_ref, the
    budget.  One object per process, computed on first use, read-only."""

    def __init__(self, ws, kind):
        self.c = C.case(ws, kind)
        v64, self.e_ref, self.errs = value_references(self.c.weights, self.c.stacks, self.c.full)
        self.budget = value_budget_of(v64, self.e_ref)
        v64.setflags(write=False)
        self.v64 = v64.reshape(C.CALLS - C.WARMUP, C.UNIQUE)

    def fault(self, f):
        got = P.network(self.c.weights, self.c.stacks, self.c.full, np.float64, P._dot64, C.FAULTS[f])[1]
        return float(np.abs(got - self.v64.reshape(-1)).max())

    def values_for(self, n):
        return self.v64[:, C.spread(C.UNIQUE, n)]


def value_case(ws, kind):
    if (ws, kind) not in _cache:
        _cache[(ws, kind)] = ValueCase(ws, kind)
    return _cache[(ws, kind)]


def judge_values(tag, vc, got, n):
    """The device's values [CALLS - WARMUP, n] of a batch against float64: prints the measured line (pytest -s), asserts error <= budget."""
    want = vc.values_for(n)
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print("f64 value %s %s/%s n %d: device error %.3g  e_ref %.3g (%s)  budget %.3g  error / budget %.3g  largest |value| %.3g" % (
        tag, vc.c.name, vc.c.kind, n, err, vc.e_ref, " ".join("%s %.2g" % kv for kv in vc.errs.items()), vc.budget, err / vc.budget,
        np.abs(want).max()))
    assert err <= vc.budget, (tag, vc.c.name, vc.c.kind, n, err, vc.budget)
    return err


# ---- the recorded batches of tests/golden: (name, weights, full, stacks, recorded values), the rows test_policy_f64_reference.py compares
RECORDED_STEP = 8  # every 8th step of the recorded games


def recorded_light(name):
    """(weights, frames [401, 6, 42, 42], compared steps, the recorded values at those steps [steps, 6], the 16 noise stacks, their values)"""
    g = np.load(os.path.join(GOLD, "policy_light.npz"))
    frames = g[name + "_frames"]
    steps = np.arange(0, frames.shape[0], RECORDED_STEP)
    return C.shipped(name), frames, steps, g[name + "_values"][steps], g["noise"], g[name + "_noise_values"]


def recorded_full():
    from tests.policy_full_weights import make_stacks, make_weights

    g = np.load(os.path.join(GOLD, "policy_full.npz"))
    return make_weights(int(g["weight_seed"])), make_stacks(int(g["stack_seed"]), g["values"].shape[0]), g["values"]


def recorded_budget(wts, stacks, full, recorded):
    """(float64 values, budget) of a recorded batch: BLAS order, sequential order and the recording itself are its references"""
    v64, e_ref, errs = value_references(wts, stacks, full, recorded=recorded)
    return v64, value_budget_of(v64, e_ref), errs


def ulp_err(got, want):
    """|got - want| in float32 ulps of max(1, |want|)"""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.maximum(np.abs(want), 1.0).astype(np.float32)).astype(np.float64)

"""The rollout heads' rules that need no GPU (include/crl.h "rollout heads"): the critic value's error budget and the fault models it
detects (tests/rollout_cases.py; the device side is tests/test_hip_rollout.py), rules.rollout_logp_reference's known answers, and
the five new entry points across the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import policy_f64_cases as C
from tests import rollout_cases as R

CASES = sorted(C.ALL_CASES)


def test_the_budget_factor_is_within_what_the_rule_allows():
    assert 2 <= R.FACTOR <= 4


@pytest.mark.parametrize("ws,kind", CASES)
def test_value_budget_and_fault_claims(ws, kind):
    """The budget comes from references only; every fault model a batch claims for the value misses it by a factor of two at least."""
    vc = R.value_case(ws, kind)
    assert "critic_w" in vc.c.weights  # (selector and wide sets: their base set's critic)
    assert vc.budget >= R.FACTOR * vc.e_ref and vc.budget >= 2 * C.ulp32(np.abs(vc.v64).max())
    assert 1e-7 < vc.budget < 1e-3, vc.budget
    ratios = {f: vc.fault(f) / vc.budget for f in R.VALUE_CLAIMS[(ws, kind)]}
    print("value %s/%s: e_ref %.3g (%s) budget %.3g largest |value| %.3g fault / budget %s" % (
        ws, kind, vc.e_ref, " ".join("%s %.2g" % kv for kv in vc.errs.items()), vc.budget, np.abs(vc.v64).max(),
        " ".join("%s %.2f" % kv for kv in ratios.items())))
    for f, r in ratios.items():
        assert r >= 2, (ws, kind, f, r)


def test_the_claims_are_the_table_the_lab_notes_state():
    assert all("b" in R.VALUE_CLAIMS[k] for k in C.LIGHT_CASES) and all("c" not in R.VALUE_CLAIMS[k] for k in C.LIGHT_CASES)
    assert all({"b", "c"} <= set(R.VALUE_CLAIMS[k]) for k in C.FULL_CASES)
    assert sorted(k for k, v in R.VALUE_CLAIMS.items() if "a" in v) == sorted(
        [("weak", "dense"), ("medium", "dense"), ("light_selector", "sparse"), ("full_selector", "dense"), ("full_selector", "sparse")])
    assert set(R.VALUE_CLAIMS) == set(C.ALL_CASES)


@pytest.mark.parametrize("name", ["weak", "medium"])
def test_recorded_light_values_lie_within_their_batches_budget(name):
    """The recording is a reference of its batch: by the rule it cannot miss the budget; what the batch's budget IS is printed."""
    w, frames, steps, rec, noise, noise_rec = R.recorded_light(name)
    stacks = C.stacks_of(frames)[steps].reshape(-1, 4, 42, 42)
    for st, r in ((stacks, rec.reshape(-1)), (noise, noise_rec)):
        v64, budget, errs = R.recorded_budget(w, st, False, r)
        print(name, len(st), "rows:", errs, "budget", budget)
        assert np.abs(r - v64).max() <= budget < 1e-4


def test_recorded_full_size_values_lie_within_their_batches_budget():
    w, st, rec = R.recorded_full()
    v64, budget, errs = R.recorded_budget(w, st, True, rec)
    print("full", errs, "budget", budget)
    assert np.abs(rec - v64).max() <= budget < 1e-4


# ---- rollout_logp_reference
def test_logp_reference_known_answers():
    from competitive_rl_amd.rules import rollout_logp_reference as ref

    eq = np.full((5, 3), 0.75, np.float32)
    assert np.array_equal(ref(eq, [0, 1, 2, 1, 0], 1.0), np.full(5, -np.log(3.0)))
    gap = np.float32(100.0)
    lg = np.array([[3.25, 3.25 + gap, 3.25]], np.float32)
    g32 = float(np.float32(lg[0, 1] - lg[0, 0]))
    assert ref(lg, [1], 1.0)[0] == 0.0
    assert ref(lg, [0], 1.0)[0] == -g32 and ref(lg, [2], 1.0)[0] == -g32
    rs = np.random.RandomState(0)
    lg = (rs.standard_normal((64, 3)) * 3).astype(np.float32)
    a = rs.randint(0, 3, 64)
    assert np.array_equal(ref(lg, a, 0.0), ref(lg, a, 1.0))  # temperature 0 = temperature 1
    # temperature 2: z is half the logits bit for bit, so the answer is that of the halved logits at temperature 1
    assert np.array_equal(ref(lg, a, 2.0), ref((lg * np.float32(0.5)).astype(np.float32), a, 1.0))
    # a probability: the three log-probs of a row exponentiate to 1
    p = sum(np.exp(ref(lg, np.full(64, k), 0.7)) for k in range(3))
    assert np.abs(p - 1).max() < 1e-12
    # float32 steps: z = l * float32(1 / T) rounded to float32, not l / T in double
    t = 3.0
    z = (lg * (np.float32(1) / np.float32(t))).astype(np.float32)
    d = (z - z.max(1, keepdims=True)).astype(np.float64)
    want = d[np.arange(64), a] - np.log(np.exp(d[:, 0]) + np.exp(d[:, 1]) + np.exp(d[:, 2]))
    assert np.array_equal(ref(lg, a, t), want)
    with pytest.raises(ValueError):
        ref(lg, a, -1.0)
    with pytest.raises(ValueError):
        ref(lg, np.full(64, 3), 1.0)
    with pytest.raises(ValueError):
        ref(lg[:, :2], a, 1.0)


# ---- ABI
NEW = ("crl_policy_set_critic", "crl_policy_act_rollout", "crl_policy_load_weights", "crl_pool_load_light", "crl_pool_load_full")


def test_the_five_entry_points_are_declared_bound_and_exported():
    from competitive_rl_amd import _native as N

    hdr = open(os.path.join(C.ROOT, "include", "crl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = N.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in N.SYMBOLS and hasattr(L, name), name
    assert [len(N.SIGNATURES[n][1]) for n in NEW] == [3, 10, 12, 9, 11]
    # the league's surface stays the thirteen entry points it was
    assert len([s for s in N.SYMBOLS if s.startswith("crl_league_")]) == 13
    assert "rollout heads" in hdr and "Epsilon is NOT folded" in hdr


def test_null_arguments_are_refused_before_any_gpu_call():
    from competitive_rl_amd import _native as N

    L = N.load()
    x = np.zeros(4, np.float32).ctypes.data_as(ctypes.c_void_p)
    for fn, args in ((L.crl_policy_set_critic, (None, x, x)),
                     (L.crl_policy_act_rollout, (None, x, 1764, None, x, 1, None, None, None, None)),
                     (L.crl_policy_load_weights, (None, x, x, x, x, None, None, x, x, None, None, None)),
                     (L.crl_pool_load_light, (None, 0, x, x, x, x, x, x, None)),
                     (L.crl_pool_load_full, (None, 0, x, x, x, x, x, x, x, x, None))):
        assert fn(*args) == -1
        assert fn.__name__.encode() in L.crl_last_error(), (fn.__name__, L.crl_last_error())

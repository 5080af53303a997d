"""The float64 forward pass of the CNN opponents (oracle/policy_oracle.py: forward64, forward_seq32) and the error budget that
tests/test_hip_policy_f64.py holds the device kernels to (tests/policy_f64_cases.py).  No GPU.

Reference checks: forward64 reproduces the logits recorded from the reference's torch modules (both golden files) within the budget
of those batches; BLAS order and sequential order are two different float32 roundings of it.

Fault models, the proof that the GPU tests can fail: (a) conv1's weights float32(w / 255) cut to two of their three bf16 terms, (b)
conv2's and (c) conv3's operands rounded to 16 significand bits, each applied inside the float64 forward.  THE INVARIANT: on every
batch that the GPU tests rely on for a fault, that fault's error is at least 2 x budget on some row -- a correct kernel <= budget <
half of every fault.  It must keep passing if policy_f64_cases.FACTOR is ever raised.  No fault was dropped: (a) separates on the
shipped light weights with all-255 and noise stacks and on the selector sets (a logit = one conv1 output), (b) and (c) on
make_weights(5) directly; whole-network input through make_weights(5) does not separate (a) (clearance 1.2 - 1.6), so no batch
claims it there."""
import os

import numpy as np
import pytest

from oracle import policy_oracle as P
from tests import policy_f64_cases as C
from tests.policy_full_weights import make_stacks, make_weights

GOLD = os.path.join(C.ROOT, "tests", "golden")


def test_the_budget_factor_is_within_what_the_rule_allows():
    assert 2 <= C.FACTOR <= 4


@pytest.mark.parametrize("name", ["weak", "medium"])
def test_forward64_reproduces_the_recorded_light_logits(name):
    """Every 8th step of the recorded game (stacks rebuilt from the recorded frames, zero planes before the first) and the 16 noise
    stacks: the recorded torch logits are a third float32 order of the batch."""
    g = np.load(os.path.join(GOLD, "policy_light.npz"))
    w = C.shipped(name)
    steps = np.arange(0, g[name + "_frames"].shape[0], 8)
    stacks = C.stacks_of(g[name + "_frames"])[steps].reshape(-1, 4, 42, 42)
    batches = ((stacks, g[name + "_logits"][steps].reshape(-1, 3), g[name + "_values"][steps].reshape(-1)),
               (g["noise"], g[name + "_noise_logits"], g[name + "_noise_values"]))
    for st, rec, rec_values in batches:
        l64, e_ref, errs = C.references(w, st, False, recorded=rec)
        budget = C.budget_of(l64, e_ref)
        print(name, len(st), "rows:", errs, "budget", budget)
        assert np.abs(rec - l64).max() <= budget
        clear = C.clear_rows(l64, budget)
        assert np.array_equal(l64.argmax(1)[clear], rec.argmax(1)[clear]) and clear.mean() > 0.99
        # float32 roundings of the same network: far inside the 1e-4 of the older tests; the critic head as well
        assert e_ref < 1e-4 and np.abs(P.forward64(w, st)[1] - rec_values).max() < 1e-4


def test_forward64_reproduces_the_recorded_full_size_logits():
    g = np.load(os.path.join(GOLD, "policy_full.npz"))
    w, st = make_weights(int(g["weight_seed"])), make_stacks(int(g["stack_seed"]), g["logits"].shape[0])
    l64, e_ref, errs = C.references(w, st, True, recorded=g["logits"])
    budget = C.budget_of(l64, e_ref)
    print("full", errs, "budget", budget)
    assert np.abs(g["logits"] - l64).max() <= budget and e_ref < 1e-4
    assert np.abs(P.forward64(w, st, True)[1] - g["values"]).max() < 1e-4
    assert np.array_equal(l64.argmax(1), g["logits"].argmax(1))


@pytest.mark.parametrize("full", [False, True])
def test_the_two_float32_orders_differ_and_bracket_nothing_else(full):
    """On dense input BLAS order and sequential order are not bit-identical (else they would be one reference, not two), both round
    the float64 logits to within e_ref by construction, and e_ref is a float32 rounding matter (a wrong layer in forward64 would not
    be)."""
    c = C.case("full" if full else "medium", "dense")
    b32, s32 = C.blas32(c.weights, c.stacks, full), P.forward_seq32(c.weights, c.stacks, full)[0]
    assert b32.dtype == s32.dtype == np.float32 and b32.shape == s32.shape == (len(c.stacks), 3)
    assert not np.array_equal(b32, s32)
    l64 = c.l64.reshape(-1, 3)
    assert max(np.abs(b32 - l64).max(), np.abs(s32 - l64).max()) == c.e_ref <= 1e-5 * max(1.0, np.abs(l64).max())
    assert P.forward64(c.weights, c.stacks, full)[0].dtype == np.float64


def test_budget_rule():
    l64 = np.array([[40.0, -3.0, 1.0]])
    assert C.budget_of(l64, 1e-5, 2) == 2e-5
    assert C.budget_of(l64, 0.0, 2) == 2 * 2.0 ** -18 == 2 * C.ulp32(40.0)  # never below two float32 ulps of the largest |logit|
    assert C.clear_rows(np.array([[0.0, 1.0, 1.0 + 3e-5], [0.0, 1.0, 1.0 + 5e-5]]), 2e-5).tolist() == [False, True]


def test_number_format_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7, 0.0, -0.0], np.float32)  # ties to even
    assert np.array_equal(C.bf16_rne(x), want) and np.signbit(C.bf16_rne(x)[-1])
    assert C.round_bits(1.0 + 2.0 ** -15 + 2.0 ** -17, 16) == 1.0 + 2.0 ** -15 and C.round_bits(0.0, 16) == 0.0
    assert C.round_bits(-3.0 * (1.0 + 2.0 ** -30), 16) == -3.0


@pytest.mark.parametrize("ws", ["weak", "medium", "full", "light_wide"])
def test_the_three_term_split_of_conv1_is_exact(ws):
    """float32(w / 255) = t0 + t1 + t2 with three RNE bf16 terms and residual zero -- for the shipped weights, make_weights and the
    wide-range set (magnitudes 2^-20 .. 2^3, zeros, -0.0, bf16 rounding ties); two terms are not enough."""
    w = C.weight_set(ws)[0]["conv1_w"]
    q, (t0, t1, t2), rest = C.bf16_terms(w)
    assert not rest.any()
    assert np.array_equal(t0.astype(np.float64) + t1.astype(np.float64) + t2.astype(np.float64), q.astype(np.float64))
    assert (t0.astype(np.float64) + t1.astype(np.float64) != q).any()
    for t in (t0, t1, t2):
        assert not (t.view(np.uint32) & 0xFFFF).any()  # each term is a bf16 number


def test_the_wide_range_set_holds_what_it_promises():
    w = C.wide_conv1().reshape(-1)
    mag = np.abs(w[w != 0])
    assert mag.min() < 2.0 ** -19 and mag.max() > 4.0 and (w > 0).any() and (w < 0).any()
    assert (w == 0).sum() > 100 and np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all()
    q = (w / np.float32(255.0)).astype(np.float32)
    tie = (q.view(np.uint32) & 0xFFFF) == 0x8000  # exactly half a bf16 ulp past a bf16 number
    assert tie.sum() > 50


@pytest.mark.parametrize("ws,kind", sorted(C.ALL_CASES))
def test_invariant_budget_below_half_of_every_fault(ws, kind):
    """The invariant of the module docstring on every batch of the GPU tests, and the cap on rows that the action comparison leaves
    out: at most 1 % on the shipped and make_weights sets (by the references alone), under 10 % everywhere."""
    c = C.case(ws, kind)
    assert c.budget >= 2 * C.ulp32(np.abs(c.l64).max()) and c.budget >= C.FACTOR * c.e_ref
    for f in C.ALL_CASES[(ws, kind)]:
        err = c.fault(f)
        print("invariant %s/%s: e_ref %.3g budget %.3g fault (%s) %.3g = %.1f x budget" % (ws, kind, c.e_ref, c.budget, f, err, err / c.budget))
        assert err >= 2 * c.budget, (ws, kind, f, err, c.budget)
    clear = C.clear_rows(c.l64.reshape(-1, 3), c.budget)
    assert clear.mean() > 0.9
    if ws in C.CAPPED:
        assert (~clear).mean() <= 0.01
    for n in (3, 11, 130, 2059):  # every run size shows distinct neighbours
        m = C.spread(C.UNIQUE, n)
        assert (m[1:] != m[:-1]).all() and len(set(m.tolist())) == min(n, C.UNIQUE)


@pytest.mark.parametrize("ws,kind", sorted(k for k, v in C.ALL_CASES.items() if v))
def test_the_gpu_tests_judge_accepts_the_references_and_rejects_the_faults(ws, kind):
    """judge() is what every GPU comparison goes through: fed the float32 references in place of device output it passes, fed a fault
    model's logits it raises -- at the run sizes of the GPU tests."""
    c = C.case(ws, kind)
    n = 11 if not c.full else 3
    m = C.spread(C.UNIQUE, C.UNIQUE)  # all distinct envs: the row with the largest fault error is among them
    for ref in (C.blas32(c.weights, c.stacks, c.full), P.forward_seq32(c.weights, c.stacks, c.full)[0]):
        ref = ref.reshape(C.CALLS - C.WARMUP, C.UNIQUE, 3)
        C.judge("reference as device", c, ref[:, C.spread(C.UNIQUE, n)], ref[:, C.spread(C.UNIQUE, n)].argmax(2), n)
    for f in C.ALL_CASES[(ws, kind)]:
        bad = P.network(c.weights, c.stacks, c.full, np.float64, P._dot64, C.FAULTS[f])[0].reshape(C.CALLS - C.WARMUP, C.UNIQUE, 3)
        with pytest.raises(AssertionError):
            C.judge("fault %s as device" % f, c, bad[:, m], bad[:, m].argmax(2), C.UNIQUE)


def test_every_fault_model_is_relied_on_somewhere_and_bites_both_networks():
    claimed = {(C.weight_set(ws)[1], f) for (ws, _), fs in C.ALL_CASES.items() for f in fs}
    assert claimed == {(False, "a"), (True, "a"), (True, "b"), (True, "c")}
    c = C.case("full", "dense")  # whole-network input through make_weights does not separate (a): it must not be claimed there
    assert "a" not in C.ALL_CASES[("full", "dense")] and c.fault("a") < 2 * c.budget


@pytest.mark.parametrize("ws", ["medium", "full"])
def test_exact_cases_on_the_references(ws):
    """actor_w = 0: the logits are actor_b (numerically: -0.0 + 0.0 is +0.0 in every statement of the network) and the first index of
    the maximum plays.  Impulses: every single pixel moves the float64 logits by far more than the budget of its two-row batch, so a
    kernel that misses or misplaces one fails the GPU test."""
    w, full = C.weight_set(ws)
    st = C.batch_of("dense", 2)[1][:2]
    for bias, act in zip(C.TIE_BIASES, C.TIE_ACTIONS):
        for fwd in (P.forward64, P.forward_seq32):
            lg = fwd(C.tie_weights(w, bias), st, full)[0]
            assert np.array_equal(lg, np.broadcast_to(np.array(bias), lg.shape)) and (lg.argmax(1) == act).all()
    d, budgets = C.impulse_reference(w, full)
    assert d.shape == (24, 3) and (np.abs(d).max(1) > 100 * budgets).all()

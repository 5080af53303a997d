"""Weight sets, input batches, the error budget and the fault models shared by tests/test_policy_f64_reference.py (CPU) and
tests/test_hip_policy_f64.py (GPU): the CNN opponents' logits against a float64 forward pass.

THE BUDGET of a batch is a rule over references only (never over device output):
    e_ref  = the largest |r - forward64| over rows and logits, r over the float32 references of the batch: BLAS order
             (policy_oracle.forward / forward_full), strictly sequential order (forward_seq32) and, on golden batches, the logits
             recorded from the reference's torch module;
    budget = FACTOR * e_ref, and never below 2 float32 ulps of the batch's largest |logit|.
The device's summation order is neither reference order, hence a factor; docs/LAB_NOTES_policy_numerics.md has the measured table.
The invariant (test_policy_f64_reference.py): a correct kernel <= budget < half of every fault model's error on the batches that
claim to detect that fault.
"""
import os

import numpy as np

from oracle import policy_oracle as P
from tests.policy_full_weights import make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 2
CALLS = 7  # frames pushed per run: calls 3 .. 6 see four made-up planes with the ring head in every position


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def blas32(wts, stacks, full):
    return (P.forward_full if full else P.forward)(wts, stacks)[0]


def references(wts, stacks, full, recorded=None):
    """(forward64 logits, e_ref, {reference name: its largest error}) of one batch of stacks [B, 4, 42, 42]."""
    l64 = P.forward64(wts, stacks, full)[0]
    errs = {"blas32": float(np.abs(blas32(wts, stacks, full) - l64).max()),
            "seq32": float(np.abs(P.forward_seq32(wts, stacks, full)[0] - l64).max())}
    if recorded is not None:
        errs["recorded"] = float(np.abs(np.asarray(recorded, np.float64) - l64).max())
    return l64, max(errs.values()), errs


def budget_of(l64, e_ref, factor=FACTOR):
    return max(factor * e_ref, 2 * ulp32(np.abs(l64).max()))


def clear_rows(l64, budget):
    """rows whose float64 top-two gap exceeds 2 x budget: there the device's argmax must be the float64 argmax"""
    srt = np.sort(l64, axis=1)
    return (srt[:, 2] - srt[:, 1]) > 2 * budget


# ---- number formats
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_terms(w):
    """The kernels' split of conv1's weights (pong_policy.hip, pong_policy_full.hip): float32(w / 255) as three bf16 terms and the
    residual left after them (all float32; the subtractions are exact)."""
    q = (np.asarray(w, np.float32) / np.float32(255.0)).astype(np.float32)
    t0 = bf16_rne(q)
    r1 = (q - t0).astype(np.float32)
    t1 = bf16_rne(r1)
    r2 = (r1 - t1).astype(np.float32)
    t2 = bf16_rne(r2)
    return q, (t0, t1, t2), (r2 - t2).astype(np.float32)


def round_bits(x, bits):
    """x rounded to `bits` significand bits (float64 in, float64 out)"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


# ---- fault models: what a subtly wrong kernel would compute, inside the float64 forward
def fault_two_terms(name, a, w):
    """(a) conv1 with the third bf16 term of w / 255 lost"""
    if name != "conv1":
        return a, w
    _, (t0, t1, _), _ = bf16_terms(w.astype(np.float32))
    return a, 255.0 * (t0.astype(np.float64) + t1.astype(np.float64))


def fault_16bit(layer):
    """(b), (c): the operands of `layer` (activations and weights) rounded to 16 significand bits"""
    def operands(name, a, w):
        return (round_bits(a, 16), round_bits(w, 16)) if name == layer else (a, w)
    return operands


FAULTS = {"a": fault_two_terms, "b": fault_16bit("conv2"), "c": fault_16bit("conv3")}


def fault_error(fault, wts, stacks, full, l64):
    return float(np.abs(P.network(wts, stacks, full, np.float64, P._dot64, FAULTS[fault])[0] - l64).max())


# ---- weight sets
# Two selected features are often both 0 behind the ReLU: distinct actor biases keep such rows from being ties that the action
# comparison would have to leave out.
SELECTOR_ACTOR_B = np.array([0.0, 0.25, 0.5], np.float32)


def shipped(name):
    return P.load_weights(os.path.join(ROOT, "competitive_rl_amd", "assets", "pong_policy_%s.npz" % name))


def wide_conv1(seed=11):
    """conv1 weights [16, 4, 4, 4] with a wide dynamic range: magnitudes 2^-20 .. 2^3, both signs, zeros, -0.0, and values whose
    w / 255 lies exactly between two bf16 numbers (a 9-bit significand ending in 1: w = 255 q is exact in float32, so w / 255 = q)."""
    rs = np.random.RandomState(seed)
    w = (rs.choice([-1.0, 1.0], 1024) * 2.0 ** rs.uniform(-20, 3, 1024)).astype(np.float32)
    kind = rs.randint(0, 8, 1024)
    w[kind == 0] = 0.0
    w[kind == 1] = -0.0
    tie = kind == 2
    q = (1.0 + (2 * rs.randint(0, 128, 1024) + 1) / 256.0) * 2.0 ** rs.randint(-12, -4, 1024) * rs.choice([-1.0, 1.0], 1024)
    w[tie] = (255.0 * q[tie]).astype(np.float32)
    assert np.array_equal((w[tie] / np.float32(255.0)).astype(np.float64), q[tie])
    return w.reshape(16, 4, 4, 4)


def selector_full(seed=3):
    """Full-size weights that isolate conv1: conv2 copies act1[oc % 16] at its centre tap, conv3 copies one act2 value per feature
    (a seeded position), their biases 0; the actor picks three features: a logit is one conv1 output of make_weights(5) plus actor_b."""
    rs = np.random.RandomState(seed)
    w = make_weights(5)
    w["conv2_w"] = np.zeros_like(w["conv2_w"])
    w["conv2_w"][np.arange(32), np.arange(32) % 16, 2, 2] = 1.0
    w["conv3_w"] = np.zeros_like(w["conv3_w"])
    w["conv3_w"][np.arange(256), np.arange(256) % 32, rs.randint(0, 10, 256), rs.randint(0, 10, 256)] = 1.0  # (row / column 10 read the padding)
    for k in ("conv2_b", "conv3_b"):
        w[k] = np.zeros_like(w[k])
    w["actor_w"] = np.zeros_like(w["actor_w"])
    w["actor_w"][np.arange(3), rs.choice(256, 3, replace=False)] = 1.0
    w["actor_b"] = SELECTOR_ACTOR_B.copy()
    return w


def selector_light(seed=4):
    """LightActorCritic weights that isolate conv1: MEDIUM's conv1, conv2 copies channel oc of the top-left conv1 output of its 2 x 2
    block (bias 0), the actor picks three features: a logit is one conv1 output plus actor_b."""
    rs = np.random.RandomState(seed)
    w = shipped("medium")
    w["conv2_w"] = np.zeros_like(w["conv2_w"])
    w["conv2_w"][np.arange(16), np.arange(16), rs.randint(0, 2, 16), rs.randint(0, 2, 16)] = 1.0
    w["actor_w"] = np.zeros_like(w["actor_w"])
    w["actor_w"][np.arange(3), rs.choice(1600, 3, replace=False)] = 1.0
    w["conv2_b"] = np.zeros_like(w["conv2_b"])
    w["actor_b"] = SELECTOR_ACTOR_B.copy()
    return w


def weight_set(name):
    """name -> (weights, full)"""
    if name in ("weak", "medium"):
        return shipped(name), False
    if name == "light_wide":
        return {**shipped("medium"), "conv1_w": wide_conv1()}, False
    if name == "light_selector":
        return selector_light(), False
    if name == "full":
        return make_weights(5), True
    if name == "full_selector":
        return selector_full(), True
    if name == "full_wide":
        return {**make_weights(5), "conv1_w": wide_conv1()}, True
    raise KeyError(name)


# ---- inputs: frames [CALLS, n, 42, 42] pushed one per call; the stack of call t is the last four frames, oldest first, zeros before
def frames_of(kind, n, seed=0):
    rs = np.random.RandomState(1000 + seed)
    if kind == "ones":
        return np.full((CALLS, n, 42, 42), 255, np.uint8)
    if kind == "dense":
        return rs.randint(0, 256, (CALLS, n, 42, 42)).astype(np.uint8)
    if kind == "bright":
        return rs.randint(192, 256, (CALLS, n, 42, 42)).astype(np.uint8)
    if kind == "sparse":
        return ((rs.random_sample((CALLS, n, 42, 42)) > 0.8) * 255).astype(np.uint8)
    raise KeyError(kind)


def stacks_of(frames):
    """[T, n, 42, 42] -> [T, n, 4, 42, 42]: what the policy's own frame stack holds at each call, starting from a zero ring"""
    T, n = frames.shape[:2]
    padded = np.concatenate([np.zeros((3, n, 42, 42), np.uint8), frames])
    return np.stack([padded[t:t + 4].transpose(1, 0, 2, 3) for t in range(T)])


WARMUP = 3  # calls whose stack still holds planes of the zeroed ring: run, not compared


def batch_of(kind, n, seed=0):
    """(frames [CALLS, n, 42, 42], stacks [(CALLS - WARMUP) * n, 4, 42, 42] of the compared calls, call-major)"""
    frames = frames_of(kind, n, seed)
    return frames, stacks_of(frames)[WARMUP:].reshape(-1, 4, 42, 42)


def spread(unique, n):
    """Row map of a large batch built from `unique` distinct envs: env i shows env (7 i) mod unique (unique is odd and no multiple of 7,
    so neighbours differ and every group of 5 or 8 envs mixes rows): the references are computed once per distinct env."""
    return (7 * np.arange(n)) % unique


# ---- the batches: (weight set, input kind) -> the fault models it is relied on to detect.  Every one is UNIQUE distinct envs over
# CALLS calls; a run at n envs shows env (7 i) mod UNIQUE in row i (spread).  Batches with "" are logits-and-action checks only: the
# references do not separate a fault model there (measured on the CPU, docs/LAB_NOTES_policy_numerics.md).
UNIQUE = 13
LIGHT_CASES = {("weak", "ones"): "a", ("medium", "ones"): "a", ("weak", "dense"): "a", ("weak", "bright"): "a",
               ("light_selector", "dense"): "a", ("light_selector", "sparse"): "a",
               ("medium", "sparse"): "", ("medium", "dense"): "", ("light_wide", "dense"): ""}
FULL_CASES = {("full", "dense"): "bc", ("full", "sparse"): "bc", ("full_selector", "dense"): "a", ("full_selector", "sparse"): "a",
              ("full_wide", "dense"): "bc"}
ALL_CASES = {**LIGHT_CASES, **FULL_CASES}
CAPPED = {"weak", "medium", "full"}  # weight sets on which at most 1 % of the rows may be left out of the action comparison

_cache = {}


class Case:
    """One batch: weights, frames [CALLS, UNIQUE, 42, 42] and, computed on first use (the child processes of the GPU tests only feed
    frames), the float64 logits [CALLS - WARMUP, UNIQUE, 3] of the compared calls, e_ref and the budget.  One object per process,
    shared by every test that needs it; its arrays are read-only."""

    def __init__(self, ws, kind):
        self.name, self.kind = ws, kind
        self.weights, self.full = weight_set(ws)
        self.frames, self.stacks = batch_of(kind, UNIQUE)
        self.frames.setflags(write=False), self.stacks.setflags(write=False)
        self._refs = None

    def _get(self, i):
        if self._refs is None:
            l64, e_ref, errs = references(self.weights, self.stacks, self.full)
            l64.setflags(write=False)
            self._refs = (l64.reshape(CALLS - WARMUP, UNIQUE, 3), e_ref, errs, budget_of(l64, e_ref))
        return self._refs[i]

    l64 = property(lambda self: self._get(0))
    e_ref = property(lambda self: self._get(1))
    errs = property(lambda self: self._get(2))
    budget = property(lambda self: self._get(3))

    def fault(self, f):
        return fault_error(f, self.weights, self.stacks, self.full, self.l64.reshape(-1, 3))

    def frames_for(self, n):
        return np.ascontiguousarray(self.frames[:, spread(UNIQUE, n)])

    def logits_for(self, n):
        return self.l64[:, spread(UNIQUE, n)]


def case(ws, kind):
    if (ws, kind) not in _cache:
        _cache[(ws, kind)] = Case(ws, kind)
    return _cache[(ws, kind)]


def judge(tag, c, got_logits, got_actions, n, rows=None):
    """The device's logits [CALLS - WARMUP, n, 3] and actions [CALLS - WARMUP, n] of batch `c` (on `rows` only: the rows of a league
    that this weight set serves) against float64: prints the measured line (pytest -s), asserts error <= budget and the float64
    argmax on every row whose top-two gap exceeds 2 x budget."""
    want = c.logits_for(n)
    if rows is not None:
        want, got_logits, got_actions = want[:, rows], np.asarray(got_logits)[:, rows], np.asarray(got_actions)[:, rows]
    err = float(np.abs(np.asarray(got_logits, np.float64) - want).max())
    clear = clear_rows(want.reshape(-1, 3), c.budget).reshape(want.shape[:2])
    print("f64 %s %s/%s n %d: device error %.3g  e_ref %.3g (%s)  budget %.3g  largest |logit| %.3g  rows compared %d of %d" % (
        tag, c.name, c.kind, n, err, c.e_ref, " ".join("%s %.2g" % kv for kv in c.errs.items()), c.budget, np.abs(want).max(),
        int(clear.sum()), clear.size))
    assert err <= c.budget, (tag, c.name, c.kind, n, err, c.budget)
    assert np.array_equal(np.asarray(got_actions)[clear], want.argmax(2)[clear]), (tag, c.name, c.kind, n)
    assert clear.mean() > 0.9
    if c.name in CAPPED:
        assert (~clear).mean() <= 0.01
    return err


# ---- exact cases
TIE_BIASES = ((0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (-0.0, 0.0, 0.0))  # first index of the maximum: 0, 0, 1, 0
TIE_ACTIONS = (0, 0, 1, 0)


def tie_weights(base, bias):
    w = dict(base)
    w["actor_w"] = np.zeros_like(base["actor_w"])
    w["actor_b"] = np.array(bias, np.float32)
    return w


IMPULSE_AT = ((0, 0), (0, 41), (41, 0), (41, 41), (41, 20), (17, 41))  # the four corners, row 41, column 41


def impulse_stacks():
    """[25, 4, 42, 42]: a zero stack with one pixel at 255, at every position of IMPULSE_AT in every plane; the last row is all zero."""
    st = np.zeros((4 * len(IMPULSE_AT) + 1, 4, 42, 42), np.uint8)
    for p in range(4):
        for i, (y, x) in enumerate(IMPULSE_AT):
            st[p * len(IMPULSE_AT) + i, p, y, x] = 255
    return st


def impulse_reference(wts, full):
    """(float64 differences logits(impulse) - logits(zero) [24, 3], the budget of each two-row batch [24])"""
    st = impulse_stacks()
    l64 = P.forward64(wts, st, full)[0]
    refs = (blas32(wts, st, full), P.forward_seq32(wts, st, full)[0])
    budgets = []
    for i in range(len(st) - 1):
        rows = [i, len(st) - 1]
        e_ref = max(float(np.abs(r[rows] - l64[rows]).max()) for r in refs)
        budgets.append(budget_of(l64[rows], e_ref))
    return l64[:-1] - l64[-1], np.array(budgets)

"""RolloutStorage (include/crl.h "rollout storage", csrc/pong_rollout.hip) on the device.

Everything is bit for bit unless a bound is stated: gathered stacks against ``policy.get_stack()`` kept after every ``act_rollout`` call and
against rules.rollout_stack_reference, scalars against what the act calls returned, advantages and returns against rules.gae_reference,
normalised advantages against the float32 rule fed the device's own statistics.  The statistics themselves against math.fsum values:
the mean within n * 2^-53 * sum|x| / n, the deviation at relative n * 2^-50 (the any-order summation bound; a factor 8 for the second pass,
the division and the root).  T = 6; N in {1, 11, 67, 130}: one env, under and over one wavefront, over two."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from competitive_rl_amd import _native as NAT  # noqa: E402
from competitive_rl_amd.rollout import RolloutBatch, RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import gae_reference, rollout_stack_reference  # noqa: E402
from tests import policy_f64_cases as C  # noqa: E402
from tests.policy_f64_child import light_policy  # noqa: E402
from tests.test_rollout_storage_rules import PATTERNS, reset_pattern  # noqa: E402

T = 6
SIZES = (1, 11, 67, 130)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _all(n):
    return torch.arange(T * n, device="cuda", dtype=torch.int64)


def _host(batch):
    return RolloutBatch(*[None if x is None else x.cpu().numpy() for x in batch])


# ---- 1. stacks and scalars through a real policy
def _play_rollout(pol, st, n, flags, rs):
    """T act_rollout calls recorded into `st` (begun by the caller): what the calls showed and returned, [T, n, ...] host arrays"""
    acts2 = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    rew2 = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    kept = {k: [] for k in ("stack", "values", "actions", "logp", "rewards", "dones")}
    for t in range(T):
        obs = torch.from_numpy(rs.randint(0, 256, (n, 1, 42, 42)).astype(np.uint8)).cuda()
        reset = torch.from_numpy(flags[t]).cuda()
        if t % 2:
            reset = reset.to(torch.uint8) * 5  # (any non-zero byte)
        values, actions, logp = pol.act_rollout(obs, reset=reset, out=acts2[:, 0])
        st.record(obs, reset, values, actions, logp)
        rew2.copy_(torch.from_numpy(rs.standard_normal((n, 2)).astype(np.float32)))
        done = torch.from_numpy(rs.random_sample(n) < 0.2).cuda()
        st.outcome(rew2[:, 0], done)
        for k, x in (("stack", pol.get_stack()), ("values", values), ("actions", actions), ("logp", logp), ("rewards", rew2[:, 0]), ("dones", done)):
            kept[k].append(x.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in kept.items()}


def _check_rollout(st, n, kept, last_values):
    f32, u8 = _host(st.gather(_all(n))), _host(st.gather(_all(n), obs_dtype=torch.uint8, fields=("obs",)))
    want = kept["stack"].reshape(T * n, 4, 42, 42)
    assert u8.obs.dtype == np.uint8 and np.array_equal(u8.obs, want)
    assert f32.obs.dtype == np.float32 and np.array_equal(f32.obs, want.astype(np.float32))
    assert np.array_equal(f32.actions, kept["actions"].reshape(-1)) and f32.actions.dtype == np.int32
    assert np.array_equal(_bits(f32.old_log_probs), _bits(kept["logp"].reshape(-1)))
    assert np.array_equal(_bits(f32.values), _bits(kept["values"].reshape(-1)))
    adv, ret = gae_reference(kept["rewards"], kept["values"], kept["dones"], last_values, st.gamma, st.gae_lambda)
    assert np.array_equal(_bits(f32.returns), _bits(ret.reshape(-1))) and np.array_equal(_bits(f32.advantages), _bits(adv.reshape(-1)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_gathered_stacks_are_what_the_policy_showed(pattern, n):
    """A light Policy fed random frames under the reset pattern; begin(policy) on a fresh policy and on one that has played three frames;
    then a second rollout (the next pattern) behind a carrying begin().  The actions go through a strided (N, 2) column, the rewards come
    from one."""
    _need_gpu()
    w = C.shipped("medium")
    second = PATTERNS[(PATTERNS.index(pattern) + 1) % len(PATTERNS)]
    for played in (0, 3):
        rs = np.random.RandomState(1000 * n + 10 * PATTERNS.index(pattern) + played)
        pol = light_policy(w, n)
        pol.set_sampling(1.0, 0.0, seed=7)
        for _ in range(played):
            pol.act_device(torch.from_numpy(rs.randint(0, 256, (n, 1, 42, 42)).astype(np.uint8)).cuda())
        st = RolloutStorage(T, n, normalize_advantage=False)
        st.begin(pol)
        for k, name in enumerate((pattern, second)):
            if k:
                st.begin()
            kept = _play_rollout(pol, st, n, reset_pattern(name, T, n, seed=n + k), rs)
            last = rs.standard_normal(n).astype(np.float32)
            st.finish(torch.from_numpy(last).cuda())
            _check_rollout(st, n, kept, last)
        st.close(), pol.close()


def test_a_fresh_storage_records_without_begin():
    """No begin at all: the zero history rows of a fresh object are the zeroed stack of a fresh policy."""
    _need_gpu()
    n = 11
    rs = np.random.RandomState(3)
    pol, st = light_policy(C.shipped("medium"), n), RolloutStorage(T, n, normalize_advantage=False)
    kept = _play_rollout(pol, st, n, reset_pattern("random", T, n, 9), rs)
    st.finish()
    _check_rollout(st, n, kept, np.zeros(n, np.float32))
    st.close(), pol.close()


# ---- 2. gather indexing against the numpy restatement
class Filled:
    """A storage of n envs filled with made-up steps behind begin(stack) (no policy), and the same data on the host"""

    def __init__(self, n, seed, p_done=0.2, normalize=False, scalars_only=False):
        """scalars_only: every frame is zero and no stack is kept on the host (a large n whose statistics are the subject)"""
        rs = np.random.RandomState(seed)
        self.n = n
        self.st = RolloutStorage(T, n, normalize_advantage=normalize)
        self.reset = reset_pattern("random", T, n, seed)
        self.actions = rs.randint(0, 3, (T, n)).astype(np.int32)
        self.values, self.logp = rs.standard_normal((T, n)).astype(np.float32), -rs.random_sample((T, n)).astype(np.float32)
        self.rewards = rs.standard_normal((T, n)).astype(np.float32)
        self.dones = np.ones((T, n), bool) if p_done >= 1 else rs.random_sample((T, n)) < p_done
        self.last = rs.standard_normal(n).astype(np.float32)
        if scalars_only:
            zero = torch.zeros((n, 1, 42, 42), dtype=torch.uint8, device="cuda")
        else:
            stack = rs.randint(1, 256, (n, 4, 42, 42)).astype(np.uint8)
            self.frames = rs.randint(0, 256, (T, n, 42, 42)).astype(np.uint8)
            self.st.begin(torch.from_numpy(stack).cuda())
            self.stacks = rollout_stack_reference(np.concatenate([np.moveaxis(stack[:, 1:], 1, 0), self.frames]), self.reset)[0].reshape(T * n, 4, 42, 42)
        for t in range(T):
            self.st.record(zero if scalars_only else torch.from_numpy(self.frames[t][:, None]).cuda(), torch.from_numpy(self.reset[t]).cuda(),
                           torch.from_numpy(self.values[t]).cuda(), torch.from_numpy(self.actions[t]).cuda(), torch.from_numpy(self.logp[t]).cuda())
            self.st.outcome(torch.from_numpy(self.rewards[t]).cuda(), torch.from_numpy(self.dones[t]).cuda())
        self.st.finish(torch.from_numpy(self.last).cuda())

    def gae(self, gamma=None, lam=None):
        adv, ret = gae_reference(self.rewards, self.values, self.dones, self.last, self.st.gamma if gamma is None else gamma,
                                 self.st.gae_lambda if lam is None else lam)
        return adv.reshape(-1), ret.reshape(-1)

    def check(self, idx, batch, adv=None):
        """`batch` (host) against plain numpy indexing by `idx`; fields that are None are skipped"""
        a, r = self.gae()
        want = RolloutBatch(self.stacks[idx], self.actions.reshape(-1)[idx], self.logp.reshape(-1)[idx], self.values.reshape(-1)[idx], r[idx],
                            (a if adv is None else adv)[idx])
        for name, g, w in zip(RolloutBatch._fields, batch, want):
            if g is None:
                continue
            if name == "obs":
                assert np.array_equal(g, w.astype(g.dtype)), name
            elif name == "actions":
                assert np.array_equal(g, w), name
            else:
                assert np.array_equal(_bits(g), _bits(w)), name


@pytest.mark.parametrize("n", [11, 67])
def test_gather_indexing(n):
    """B in {1, 63, 64, 65, T * N}; reversed, shuffled and one-index-repeated orders; each optional output left out in turn; `out` reused."""
    _need_gpu()
    f = Filled(n, 40 + n)
    total = T * n
    rs = np.random.RandomState(n)
    orders = {"reversed": np.arange(total)[::-1].copy(), "shuffled": rs.permutation(total), "repeated": np.full(65, total - 3)}
    for b in (1, 63, 64, 65, total):
        orders["first_%d" % b] = np.arange(b)
        orders["shuffled_%d" % b] = rs.permutation(total)[:b] if b <= total else rs.randint(0, total, b)
    for name, idx in orders.items():
        dev = torch.from_numpy(idx.astype(np.int64)).cuda()
        f.check(idx, _host(f.st.gather(dev)))
        f.check(idx, _host(f.st.gather(dev, obs_dtype=torch.uint8)))
    idx = orders["shuffled_65"]
    dev = torch.from_numpy(idx.astype(np.int64)).cuda()
    for leave_out in RolloutBatch._fields:
        fields = [k for k in RolloutBatch._fields if k != leave_out]
        got = f.st.gather(dev, fields=fields)
        assert getattr(got, leave_out) is None and all(getattr(got, k) is not None for k in fields)
        f.check(idx, _host(got))
    out = f.st.empty_batch(65)
    assert f.st.gather(dev, out=out) is out
    f.check(idx, _host(out))
    idx2 = orders["first_65"]
    f.st.gather(torch.from_numpy(idx2.astype(np.int64)).cuda(), out=out)
    f.check(idx2, _host(out))
    sizes = [b.obs.shape[0] for b in f.st.minibatches(4)]
    assert sizes == [total // 4] * 4
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    seen = np.concatenate([b.actions.cpu().numpy() for b in f.st.minibatches(2, generator=g, obs_dtype=torch.uint8)])
    g.manual_seed(5)
    perm = torch.randperm(total, device="cuda", generator=g).cpu().numpy()
    assert np.array_equal(seen, f.actions.reshape(-1)[perm[:2 * (total // 2)]])
    f.st.close()


def test_offsets_past_32_bits():
    """65 536 envs x 38 steps: the plane rows end 4.77 GB into the array, and a float32 gather of 80 000 samples ends 2.26 GB into its
    output -- byte offsets that fit neither an int32 nor (the rows) a uint32.  Checked on the device against the last four frames.

    Memory: 4.84 GB of storage, 2.26 GB each for the gathered batch and its reference, about 1.5 GB of frames and intermediates: 11 GB
    of free device memory, asserted below so that a smaller (or busier) card says so and not `out of memory` somewhere inside."""
    _need_gpu()
    n, steps, b = 65536, 38, 80000
    free, need = torch.cuda.mem_get_info()[0], 11 * 10 ** 9
    assert free >= need, f"test_offsets_past_32_bits needs {need / 1e9:.0f} GB of free device memory, this device has {free / 1e9:.1f} GB free"
    st = RolloutStorage(steps, n, normalize_advantage=False)
    assert (steps + 3) * n * 1776 > 2 ** 32 and b * 4 * 42 * 42 * 4 > 2 ** 31
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    last4, zero_r = [], torch.zeros(n, device="cuda")
    none = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for t in range(steps):
        obs = torch.randint(0, 256, (n, 1, 42, 42), device="cuda", dtype=torch.uint8, generator=g)
        st.record(obs, None, None, None, None)
        st.outcome(zero_r, none)
        last4 = (last4 + [obs])[-4:]
    st.finish()
    envs = torch.randint(0, n, (b,), device="cuda", generator=g)
    envs[0], envs[-1] = n - 1, 0
    got = st.gather((steps - 1) * n + envs, fields=("obs",)).obs
    want = torch.cat(last4, dim=1)[envs].float()
    assert torch.equal(got, want)
    st.close()


# ---- 3. GAE
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("p_done", [0.2, 0.0, 1.0])
def test_gae_bit_for_bit(p_done, n):
    _need_gpu()
    f = Filled(n, 70 + n, p_done=p_done)
    assert f.dones.all() if p_done >= 1 else (not f.dones.any() if p_done == 0 else True)
    idx = np.arange(T * n)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        f.st.gamma, f.st.gae_lambda = gamma, lam
        f.st.finish(torch.from_numpy(f.last).cuda())
        got = _host(f.st.gather(_all(n), fields=("returns", "advantages")))
        f.check(idx, got)
    f.st.close()


# ---- 4. statistics and normalisation
@pytest.mark.parametrize("n", SIZES + (11000,))
def test_statistics_and_normalised_advantages(n):
    """11 000 envs: 66 000 advantages = 258 workgroups' worth, more than the 256 the first pass launches (the strided loop)."""
    _need_gpu()
    f = Filled(n, 90 + n, normalize=True, scalars_only=n > 1000)
    count = T * n
    adv, _ = f.gae()
    x = [float(v) for v in adv]
    mean = math.fsum(x) / count
    std = math.sqrt(math.fsum((v - mean) ** 2 for v in x) / (count - 1))
    got_mean, got_std = f.st.stats()
    sum_abs = math.fsum(abs(v) for v in x)
    print("rollout statistics n %d: mean error %.3g (bound %.3g)  std relative error %.3g (bound %.3g)" % (
        n, abs(got_mean - mean), count * 2.0 ** -53 * sum_abs / count, abs(got_std - std) / std, count * 2.0 ** -50))
    assert abs(got_mean - mean) <= count * 2.0 ** -53 * sum_abs / count
    assert abs(got_std - std) <= count * 2.0 ** -50 * std
    norm = f.st.gather(_all(n), fields=("advantages",)).advantages.cpu().numpy()
    want = (adv - np.float32(got_mean)) / (np.float32(got_std) + np.float32(1e-5))
    assert want.dtype == np.float32 and np.array_equal(_bits(norm), _bits(want))
    # a second run gives the same bits
    f.st.finish(torch.from_numpy(f.last).cuda())
    assert f.st.stats() == (got_mean, got_std)
    assert np.array_equal(_bits(f.st.gather(_all(n), fields=("advantages",)).advantages.cpu().numpy()), _bits(norm))
    # normalize=False hands out the raw advantages, and there are no statistics to ask for
    f.st.normalize_advantage = False
    f.st.finish(torch.from_numpy(f.last).cuda())
    assert np.array_equal(_bits(f.st.gather(_all(n), fields=("advantages",)).advantages.cpu().numpy()), _bits(adv))
    with pytest.raises(NAT.CrlError, match="crl_rollout_stats"):
        f.st.stats()
    f.st.close()


def test_a_single_advantage_has_deviation_zero():
    """T * N = 1 (include/crl.h "Statistics"): the mean is the advantage, the deviation is 0 -- not the 0 / 0 of the unbiased formula --
    and the normalised advantage is (adv - mean32) / 1e-5f = 0."""
    _need_gpu()
    st = RolloutStorage(1, 1, gamma=0.99, gae_lambda=0.95, normalize_advantage=True)
    st.record(torch.zeros((1, 1, 42, 42), dtype=torch.uint8, device="cuda"), None, torch.full((1,), 0.25, device="cuda"), None, None)
    st.outcome(torch.full((1,), 1.5, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda"))
    st.finish()
    assert st.stats() == (1.25, 0.0)
    got = st.gather(torch.zeros(1, dtype=torch.int64, device="cuda"), fields=("advantages", "returns"))
    assert got.advantages.item() == 0.0 and got.returns.item() == 1.5
    st.close()


# ---- 5. refusals
def test_the_state_machine_refuses_and_the_object_stays_usable():
    """Every refusal is CRL_EINVAL with a message naming the call, made before any GPU call: the rollout completed around the refused
    calls gathers what it should."""
    _need_gpu()
    n = 11
    f = Filled(n, 5)  # (a finished rollout: its data is recorded a second time below, around the refusals)
    L, h, st = f.st._L, f.st._h, f.st
    s = st._stream()
    vp = ctypes.c_void_p
    frames = [torch.from_numpy(f.frames[t][:, None]).cuda() for t in range(T)]
    resets = [torch.from_numpy(f.reset[t]).cuda().view(torch.uint8) for t in range(T)]
    acts, vals, lps = ([torch.from_numpy(x[t]).cuda() for t in range(T)] for x in (f.actions, f.values, f.logp))
    rews, dones = [torch.from_numpy(f.rewards[t]).cuda() for t in range(T)], [torch.from_numpy(f.dones[t]).cuda().view(torch.uint8) for t in range(T)]
    last = torch.from_numpy(f.last).cuda()
    idx = _all(n)
    obs = torch.empty((T * n, 4, 42, 42), device="cuda")
    stats = (ctypes.c_double * 2)()

    def p(t, off=0):
        return vp(t.data_ptr() + off)

    def record(t, frame=None, stride=42 * 42, off=0, a_off=0):
        return L.crl_rollout_record(h, t, p(frames[t % T], off) if frame is None else frame, stride, p(resets[t % T]), p(acts[t % T], a_off), 1, p(vals[t % T]),
                                    p(lps[t % T]), s)

    def outcome(t, stride=1):
        return L.crl_rollout_outcome(h, t, p(rews[t % T]), stride, p(dones[t % T]), s)

    def finish():
        return L.crl_rollout_finish(h, p(last), 0.99, 0.95, 0, s)

    def gather(i=None, o=None, off=0):
        return L.crl_rollout_gather(h, p(idx) if i is None else i, idx.numel(), p(obs, off) if o is None else o, NAT.CRL_OBS_F32, None, None, None, None, None, s)

    def refused(rc, who):
        assert rc == -1 and who.encode() in L.crl_last_error() and len(L.crl_last_error()) > len(who) + 2, (rc, L.crl_last_error())

    # finished: a record needs a begin first; statistics were not computed
    refused(record(0), "crl_rollout_record")
    refused(outcome(0), "crl_rollout_outcome")
    refused(L.crl_rollout_stats(h, stats), "crl_rollout_stats")
    assert L.crl_rollout_begin(h, None, s) == 0  # carry over from the finished rollout
    refused(gather(), "crl_rollout_gather")      # begun, not finished
    refused(L.crl_rollout_begin(h, None, s), "crl_rollout_begin")  # a carrying begin on an unfinished rollout
    refused(finish(), "crl_rollout_finish")
    refused(outcome(0), "crl_rollout_outcome")   # no record yet
    refused(record(1), "crl_rollout_record")     # not the next step
    refused(record(-1), "crl_rollout_record")
    # null and misaligned pointers
    refused(record(0, frame=vp(None)), "crl_rollout_record")
    refused(record(0, off=1), "crl_rollout_record")
    refused(record(0, stride=42 * 42 + 2), "crl_rollout_record")
    refused(record(0, stride=42 * 42 - 4), "crl_rollout_record")
    refused(record(0, a_off=2), "crl_rollout_record")
    refused(L.crl_rollout_record(None, 0, p(frames[0]), 1764, None, None, 1, None, None, s), "crl_rollout_record")
    refused(L.crl_rollout_begin(h, p(obs, 1), s), "crl_rollout_begin")
    assert record(0) == 0
    refused(record(0), "crl_rollout_record")     # twice
    refused(record(2), "crl_rollout_record")
    refused(outcome(1), "crl_rollout_outcome")   # the outcome of a step without a record
    refused(L.crl_rollout_outcome(h, 0, None, 1, p(dones[0]), s), "crl_rollout_outcome")
    refused(L.crl_rollout_outcome(h, 0, p(rews[0]), 1, None, s), "crl_rollout_outcome")
    refused(outcome(0, stride=0), "crl_rollout_outcome")
    assert outcome(0) == 0
    refused(outcome(0), "crl_rollout_outcome")   # twice
    for t in range(1, T):
        if t == T - 1:
            refused(finish(), "crl_rollout_finish")
        assert record(t) == 0
        refused(finish(), "crl_rollout_finish")  # T records, T - 1 outcomes at the last step
        assert outcome(t) == 0
    refused(record(T), "crl_rollout_record")     # past the last step
    refused(gather(), "crl_rollout_gather")
    refused(L.crl_rollout_finish(h, p(last, 2), 0.99, 0.95, 0, s), "crl_rollout_finish")
    assert finish() == 0
    refused(gather(i=vp(None)), "crl_rollout_gather")
    refused(gather(i=p(idx, 4)), "crl_rollout_gather")
    refused(gather(off=4), "crl_rollout_gather")  # a float32 observation is 16-byte aligned
    refused(L.crl_rollout_gather(h, p(idx), idx.numel(), p(obs), 7, None, None, None, None, None, s), "crl_rollout_gather")
    refused(L.crl_rollout_gather(h, p(idx), -1, p(obs), NAT.CRL_OBS_F32, None, None, None, None, None, s), "crl_rollout_gather")
    refused(L.crl_rollout_stats(h, None), "crl_rollout_stats")
    out = ctypes.c_void_p()
    refused(L.crl_rollout_create(0, 0, T, ctypes.byref(out)), "crl_rollout_create")
    refused(L.crl_rollout_create(0, 1 << 20, 1 << 12, ctypes.byref(out)), "crl_rollout_create")
    refused(L.crl_rollout_create(0, n, T, None), "crl_rollout_create")
    # the rollout recorded around all this is the first one's data again, carried over from the first one's end
    rows = np.concatenate([f.frames[T - 3:], f.frames])
    depth_first = rollout_stack_reference(np.concatenate([np.zeros((3, n, 42, 42), np.uint8), f.frames]), f.reset)[1]  # (the depths do not depend on the rows)
    f.stacks = rollout_stack_reference(rows, f.reset, np.minimum(3, depth_first[-1]))[0].reshape(T * n, 4, 42, 42)
    f.check(np.arange(T * n), _host(st.gather(idx)))
    st.close()

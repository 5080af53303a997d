"""The rule of include/crl.h "sampled actions" as the package restates it in numpy (``league_sample_reference``;
tests/test_hip_league_sampling.py compares the kernels with that restatement): the generator words it uses, its frequencies, the greedy
and explore branches, the explore threshold, and the new entry points' argument checks.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from competitive_rl_amd import _native as N
from competitive_rl_amd.league import check_sampling, league_draw_reference, league_sample_reference, sample_eps_q
from tests.test_league_rules import M32, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAIN_SAMPLE = 0x4C475553  # "LGUS"
PAIRS = 200_000


def _words(seed, gid, n):
    gid, n = np.broadcast_arrays(np.asarray(gid, np.uint64), np.asarray(n, np.uint64))
    return philox4x32_10(gid & M32, gid >> np.uint64(32), n, np.full(gid.shape, DOMAIN_SAMPLE, np.uint64), int(seed) & 0xFFFFFFFF, int(seed) >> 32)


def _pairs():
    """200 000 (gid, n) pairs: 2 000 envs (ids past 2^32 among them) at 100 act calls each."""
    gid = np.concatenate([np.arange(1000), (1 << 33) + np.arange(1000)]).astype(np.uint64)
    return np.repeat(gid, 100), np.tile(np.arange(100, dtype=np.uint64), 2000)


def test_the_domain_word_is_where_the_header_says():
    hdr = open(os.path.join(ROOT, "include", "crl.h")).read()
    assert int(re.search(r"#define CRL_LEAGUE_DOMAIN_SAMPLE (0x[0-9A-Fa-f]+)u", hdr).group(1), 0) == N.CRL_LEAGUE_DOMAIN_SAMPLE == DOMAIN_SAMPLE
    assert DOMAIN_SAMPLE.to_bytes(4, "big") == b"LGUS"
    assert len({DOMAIN_SAMPLE, N.CRL_LEAGUE_DOMAIN_ACTION, N.CRL_LEAGUE_DOMAIN_OPPONENT, N.CRL_LEDGER_DOMAIN_OPPONENT, N.CRL_ARENA_DOMAIN_PAIR, 0x504F4E47}) == 6
    assert '"sampled actions"' in open(os.path.join(ROOT, "competitive_rl_amd", "csrc", "pong_sample.h")).read() and "Sampled actions" in hdr


def test_the_sample_uses_the_word_the_league_draw_uses():
    """r comes from the same x0 as ``league_draw_reference`` for the new domain: with m = 2^24 that draw is x0 >> 8.  Logits whose softmax
    boundaries sit at 0.25 and 0.75 (float64: exactly, log 2 apart) turn r back into an action."""
    gid, n = _pairs()
    for seed in (0, 11, (1 << 63) + 5):
        r24 = league_draw_reference(seed, gid, n, DOMAIN_SAMPLE, 1 << 24)
        assert np.array_equal(r24, (_words(seed, gid, n)[0] >> np.uint64(8)).astype(np.int64))
        a, explored, margin = league_sample_reference(seed, gid, n, np.log(np.array([1.0, 2.0, 1.0])), 1.0, 0.0)
        r = r24 * 2.0 ** -24
        expect = np.where(r < 0.25, 0, np.where(r < 0.75, 1, 2))
        clear = margin > 1e-12
        assert clear.mean() > 0.999 and not explored.any() and np.array_equal(a[clear], expect[clear])
        assert np.allclose(margin, np.minimum(np.abs(r - 0.25), np.abs(r - 0.75)), atol=1e-12)


def _within_4_sigma(count, total, p):
    return abs(count - total * p) <= 4.0 * np.sqrt(total * p * (1.0 - p))


@pytest.mark.parametrize("temperature", [1.0, 0.5, 2.0])
def test_action_frequencies_follow_the_softmax(temperature):
    gid, n = _pairs()
    logits = np.array([0.3, -0.9, 1.1], np.float32)
    a, explored, _ = league_sample_reference(77, gid, n, logits, temperature, 0.0)
    z = logits.astype(np.float64) * float(np.float32(1) / np.float32(temperature))
    p = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
    assert len(a) == PAIRS and not explored.any() and p.min() > 0.01
    for k in range(3):
        assert _within_4_sigma(int((a == k).sum()), PAIRS, p[k]), (k, (a == k).mean(), p[k])


def test_epsilon_explores_on_its_share_of_draws_with_uniform_actions():
    gid, n = _pairs()
    logits = np.array([5.0, 0.0, -5.0])
    a, explored, margin = league_sample_reference(3, gid, n, logits, 0.0, 0.25)
    k = int(explored.sum())
    assert _within_4_sigma(k, PAIRS, 0.25), k / PAIRS
    for v in range(3):
        assert _within_4_sigma(int((a[explored] == v).sum()), k, 1 / 3), (v, (a[explored] == v).mean())
    assert (a[~explored] == 0).all() and np.isinf(margin).all()
    # the words: explore on x1, the action from x2, integer-exact
    w = _words(3, gid, n)
    assert np.array_equal(explored, w[1] < np.uint64(1 << 30))
    assert np.array_equal(a[explored], ((w[2] * np.uint64(3)) >> np.uint64(32)).astype(np.int64)[explored])
    # with a temperature: the same draws explore, the others sample
    b, explored_t, margin_t = league_sample_reference(3, gid, n, logits, 1.0, 0.25)
    assert np.array_equal(explored_t, explored) and np.array_equal(b[explored], a[explored])
    assert np.isinf(margin_t[explored]).all() and np.isfinite(margin_t[~explored]).all()
    # epsilon 1 explores always (but for x1 = 0xFFFFFFFF, absent here), epsilon 0 never
    assert league_sample_reference(3, gid, n, logits, 1.0, 1.0)[1].all() and not league_sample_reference(3, gid, n, logits, 1.0, 0.0)[1].any()


def test_temperature_zero_is_the_first_index_argmax():
    rs = np.random.RandomState(2)
    logits = rs.randn(5000, 3).astype(np.float32)
    ties = np.array([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0], [1.0, 0.0, 1.0], [-1.0, -1.0, -2.0], [0.0, 0.0, 0.0]], np.float32)
    logits = np.concatenate([logits, ties])
    a, explored, margin = league_sample_reference(9, np.arange(len(logits)), 4, logits, 0.0, 0.0)
    assert np.array_equal(a, np.argmax(logits, axis=1)) and not explored.any() and np.isinf(margin).all()
    assert a[-6:].tolist() == [0, 1, 0, 0, 0, 0]


def test_the_explore_threshold():
    assert [sample_eps_q(e) for e in (0.0, 2.0 ** -32, 0.5, 1.0)] == [0, 1, 1 << 31, 0xFFFFFFFF]
    assert sample_eps_q(np.float32(0.1)) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))  # (from the float32 the C ABI takes)


def test_bad_play_styles_are_refused_on_the_host():
    for t, e in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1e-45, 0.0), (1.0, -0.1), (1.0, 1.5), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            check_sampling(t, e)
        with pytest.raises(ValueError):
            league_sample_reference(0, 0, 0, np.zeros(3), t, e)
    assert check_sampling(0, 0) == (0.0, 0.0) and check_sampling(2, 1) == (2.0, 1.0)


def test_the_new_exports_refuse_bad_arguments_without_gpu():
    L = N.load()
    for s in ("crl_sampling_set_agent", "crl_sampling_get_agent", "crl_policy_set_sampling"):
        assert s in N.SYMBOLS and hasattr(L, s)
    t, e = C.c_float(), C.c_float()
    assert L.crl_sampling_set_agent(None, 0, 1.0, 0.0) == -1 and b"null league" in L.crl_last_error()
    assert L.crl_sampling_get_agent(None, 0, C.byref(t), C.byref(e)) == -1 and b"null" in L.crl_last_error()
    for bad in (-0.5, float("nan"), float("inf"), 1e-45):
        assert L.crl_sampling_set_agent(None, 0, bad, 0.0) == -1 and b"temperature" in L.crl_last_error()
        assert L.crl_policy_set_sampling(None, bad, 0.0, 0, 0) == -1 and b"temperature" in L.crl_last_error()
    for bad in (-0.001, 1.001, float("nan")):
        assert L.crl_sampling_set_agent(None, 0, 1.0, bad) == -1 and b"epsilon" in L.crl_last_error()
        assert L.crl_policy_set_sampling(None, 1.0, bad, 0, 0) == -1 and b"epsilon" in L.crl_last_error()
    assert L.crl_policy_set_sampling(None, 1.0, 0.0, 0, 0) == -1 and b"null policy" in L.crl_last_error()

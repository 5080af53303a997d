"""The ledger's weighted draw and its PFSP weights (include/crl.h "ledger draws", "PFSP weights"), restated in plain numpy here --
tests/test_hip_ledger.py compares the kernels with the package's restatements, this file compares those with THIS one and with
answers worked out by hand -- and the agreement of header, ctypes binding and library for the crl_ledger_* entry points.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from competitive_rl_amd import _native as N
from competitive_rl_amd.league import league_draw_reference
from competitive_rl_amd.ledger import LeagueLedger, ledger_draw_reference, pfsp_weights_reference
from tests.test_league_rules import DOMAIN_ACTION, DOMAIN_OPPONENT, DOMAIN_SERVE, M32, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAIN_LEDGER = 0x4C475557  # "LGUW"


def weighted_draw(seed, gid, n, w):
    """r = (word 0 * T) >> 32 of counter (gid lo, gid hi, n, "LGUW"), key (seed lo, seed hi); the smallest a whose cumulative weight
    exceeds r, found by walking the table."""
    gid, n = np.broadcast_arrays(np.asarray(gid, np.uint64), np.asarray(n, np.uint64))
    x = philox4x32_10(gid & M32, gid >> np.uint64(32), n, np.full(gid.shape, DOMAIN_LEDGER, np.uint64), int(seed) & 0xFFFFFFFF, int(seed) >> 32)[0]
    total = sum(int(v) for v in w)
    assert 0 < total < 2 ** 32
    r = (x * np.uint64(total)) >> np.uint64(32)
    out, cum = np.full(gid.shape, -1, np.int64), 0
    for a, v in enumerate(w):
        cum += int(v)
        out[(out < 0) & (r < np.uint64(cum))] = a
    return out


def test_header_binding_and_library_agree_on_the_ledger():
    hdr = open(os.path.join(ROOT, "include", "crl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(crl_ledger_[a-z_0-9]+)\s*\(", code)))
    assert len(declared) >= 11 and declared == sorted(s for s in N.SYMBOLS if s.startswith("crl_ledger_"))
    for want in ("create", "destroy", "seed", "reset", "set_weights", "get_weights", "pfsp_weights", "get_counters", "set_counters", "step"):
        assert "crl_ledger_" + want in declared, want
    L = N.load()
    for s in declared:
        assert hasattr(L, s), s
    defs = dict(re.findall(r"#define (CRL_LEDGER_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)", hdr))
    assert int(defs["CRL_LEDGER_DOMAIN_OPPONENT"], 0) == N.CRL_LEDGER_DOMAIN_OPPONENT == DOMAIN_LEDGER
    assert len({DOMAIN_LEDGER, DOMAIN_OPPONENT, DOMAIN_ACTION, DOMAIN_SERVE}) == 4
    assert int(defs["CRL_LEDGER_COUNTERS"]) == N.CRL_LEDGER_COUNTERS == len(N.CRL_LEDGER_COUNTER_NAMES) == 6
    order = re.search(r"enum crl_ledger_counter \{([^}]*)\}", hdr).group(1)
    assert [x.strip().split(" = ")[0][len("CRL_LEDGER_"):].lower() for x in order.split(",")] == list(N.CRL_LEDGER_COUNTER_NAMES)
    modes = re.search(r"enum crl_ledger_pfsp \{([^}]*)\}", hdr).group(1)
    assert [tuple(x.strip().split(" = ")) for x in modes.split(",")] == [("CRL_LEDGER_PFSP_HARD", "0"), ("CRL_LEDGER_PFSP_VARIANCE", "1")]
    assert (N.CRL_LEDGER_PFSP_HARD, N.CRL_LEDGER_PFSP_VARIANCE) == (0, 1)
    # the league's own surface is what it was
    assert len([s for s in N.SYMBOLS if s.startswith("crl_league_")]) == 13


def test_ledger_entry_points_refuse_null_and_bad_arguments():
    L = N.load()
    h = ctypes.c_void_p()
    assert L.crl_ledger_create(0, 8, 0, 0, 4, None) == -1 and b"crl_ledger_create" in L.crl_last_error()
    for envs, base, agents in ((0, 0, 4), (-3, 0, 4), (1 << 31, 0, 4), (8, -1, 4), (8, 0, 0), (8, 0, 17)):
        assert L.crl_ledger_create(0, envs, base, 0, agents, ctypes.byref(h)) == -1 and b"crl_ledger_create" in L.crl_last_error()
        assert not h.value
    assert L.crl_ledger_step(None, None, None, 0, None, 0, None, None) == -1 and b"crl_ledger_step" in L.crl_last_error()
    for name, args in (("seed", (None, 0, None)), ("reset", (None, None)), ("set_agents", (None, 4, None)), ("set_weights", (None, None, 0, None)),
                       ("get_weights", (None, None, None)), ("pfsp_weights", (None, None, 0, 2, 1, None)), ("get_counters", (None, None, None, None)),
                       ("set_counters", (None, None, None, None)), ("get_env_state", (None, None, None, None, None)),
                       ("set_env_state", (None, None, None, None, None))):
        assert getattr(L, "crl_ledger_" + name)(*args) == -1 and b"crl_ledger_" + name.encode() in L.crl_last_error(), name
    L.crl_ledger_destroy(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LeagueLedger(8, 4, "cpu")
    import competitive_rl_amd as crl

    assert crl.LeagueLedger is LeagueLedger and crl.ledger_draw_reference is ledger_draw_reference


def test_unit_weights_are_the_uniform_draw_under_the_new_domain_word():
    rs = np.random.RandomState(1)
    gid, ctr = rs.randint(0, 1 << 40, 4000), rs.randint(0, 1 << 31, 4000)
    for seed in (0, 5, (1 << 63) + 77):
        for m in (1, 2, 4, 7, 16):
            got = ledger_draw_reference(seed, gid, ctr, [1] * m)
            assert np.array_equal(got, league_draw_reference(seed, gid, ctr, DOMAIN_LEDGER, m))
            assert m == 1 or not np.array_equal(got, league_draw_reference(seed, gid, ctr, DOMAIN_OPPONENT, m))


def test_package_restatement_agrees_with_the_walk_of_the_table():
    rs = np.random.RandomState(2)
    gid, ctr = rs.randint(0, 1 << 40, 3000), rs.randint(0, 1 << 31, 3000)
    for seed, w in ((3, [1, 2, 3, 0, 10]), ((1 << 63) + 9, [0, 0, 5, 0]), (8, [0xFFFFFFFF]), (8, [0x7FFFFFFF, 0, 0x7FFFFFFF, 1]),
                    (1, [65536] * 16), (4, rs.randint(0, 1000, 16).tolist())):
        assert np.array_equal(ledger_draw_reference(seed, gid, ctr, w), weighted_draw(seed, gid, ctr, w)), w


def test_known_answers():
    assert ledger_draw_reference(12345, np.arange(8), 0, [1, 2, 3, 0, 10]).tolist() == [2, 1, 4, 4, 2, 0, 4, 4]
    assert ledger_draw_reference((1 << 63) + 9, (1 << 40) + np.arange(6), np.arange(6) * 1000003, [5, 0, 0, 7]).tolist() == [0, 3, 3, 3, 3, 3]
    assert ledger_draw_reference(7, 3, np.arange(8), [0, 0, 1]).tolist() == [2] * 8
    assert ledger_draw_reference(7, np.arange(6), 2, [0xFFFFFFFF]).tolist() == [0] * 6
    assert weighted_draw(12345, np.arange(8), 0, [1, 2, 3, 0, 10]).tolist() == [2, 1, 4, 4, 2, 0, 4, 4]
    # the word the rule scales, from the generator's published vector: counter (0, 0, 0, 0) under key 0 gives 0x6627E8D5, so under
    # weights [1, 1, 1, 1] it lands in (0x6627E8D5 * 4) >> 32 = 1 (tests/test_league_rules.py test_philox_known_answers)
    assert (0x6627E8D5 * 4) >> 32 == 1
    for bad in ([0, 0, 0], [0xFFFFFFFF, 1], [], [1] * 17, [-1, 2]):
        with pytest.raises(ValueError):
            ledger_draw_reference(0, 0, 0, bad)


def test_a_zero_weight_agent_is_never_drawn():
    n = 100_000
    for w in ([3, 0, 1, 0], [0, 1, 0, 1000], [1, 0, 0, 0, 0, 0, 0, 1]):
        v = np.concatenate([ledger_draw_reference(21, np.arange(n), 0, w), ledger_draw_reference(22, 5, np.arange(n), w)])
        seen = np.bincount(v, minlength=len(w))
        assert all((seen[a] == 0) == (w[a] == 0) for a in range(len(w))), (w, seen)


def test_draws_do_not_depend_on_how_the_id_range_is_cut():
    n, ctr, w = 1003, np.arange(1003) % 5, [4, 1, 0, 7]
    whole = ledger_draw_reference(3, np.arange(n), ctr, w)
    for cut in (1, 500, 999):
        lo = ledger_draw_reference(3, np.arange(cut), ctr[:cut], w)
        hi = ledger_draw_reference(3, cut + np.arange(n - cut), ctr[cut:], w)
        assert np.array_equal(np.concatenate([lo, hi]), whole)


# 99.9 % quantiles of the chi-square distribution (standard tables), by degrees of freedom; the seeds are fixed
CHI2_999 = {1: 10.828, 2: 13.816, 3: 16.266, 4: 18.467}


@pytest.mark.parametrize("w", [[1, 2, 3, 0, 10], [1, 1, 1, 1], [100, 1, 50], [5, 0, 0, 7]])
def test_draws_follow_the_weights(w):
    """2 * 10^5 draws, over envs at one counter value and over the counter for a handful of envs, against the expected counts T * w / sum(w)."""
    n = 200_000
    w = np.asarray(w)
    expect = n * w / w.sum()
    for v in (ledger_draw_reference(2024, np.arange(n), 0, w), ledger_draw_reference(11, np.arange(16)[:, None], np.arange(n // 16)[None, :], w).reshape(-1)):
        obs = np.bincount(v, minlength=len(w)).astype(np.float64)
        assert (obs[w == 0] == 0).all()
        chi2 = ((obs - expect)[w > 0] ** 2 / expect[w > 0]).sum()
        assert chi2 < CHI2_999[int((w > 0).sum()) - 1], (w.tolist(), chi2)


def _books(episodes, wins, draws):
    c = np.zeros((N.CRL_LEDGER_COUNTERS, N.CRL_LEAGUE_MAX_AGENTS), np.int64)
    k = len(episodes)
    c[0, :k], c[1, :k], c[3, :k] = episodes, wins, draws
    c[2] = c[0] - c[1] - c[3]
    return c


def test_pfsp_weights_known_answers():
    """By hand: never played -> p = 1/2; 10 wins of 10 -> p = 11/12, 1 - p = 1/12; 0 wins of 10 -> 1 - p = 11/12; weight = floor +
    int(f * 65535): 65535 / 2 = 32767.5, 65535 / 12 = 5461.25, 65535 * 11 / 12 = 60073.75, 65535 / 4 = 16383.75."""
    c = _books([0, 10, 10, 7, 1000], [0, 10, 0, 3, 333], [0, 0, 0, 1, 1])
    assert pfsp_weights_reference(c, 5, "hard", 1, 1)[:6].tolist() == [32768, 5462, 60074, 32768, 43658, 0]
    assert pfsp_weights_reference(c, 5, "hard", 2, 1)[:6].tolist() == [16384, 456, 55068, 16384, 29084, 0]
    assert pfsp_weights_reference(c, 5, "hard", 3, 0)[:6].tolist() == [8191, 37, 50478, 8191, 19374, 0]
    assert pfsp_weights_reference(c, 5, "variance", 2, 5)[:6].tolist() == [16388, 5011, 5011, 16388, 14579, 0]
    w = pfsp_weights_reference(c, 3, "hard", 2, 1)
    assert w.dtype == np.uint32 and w.shape == (16,) and (w[3:] == 0).all() and (w[:3] > 0).all()
    # agent 3: 3 wins and 1 draw of 7 -> p = (3 + 0.5 + 1) / 9 = 1/2 exactly, like the agent never played
    assert w[0] == pfsp_weights_reference(c, 5, "hard", 2, 1)[3]
    with pytest.raises(ValueError):
        pfsp_weights_reference(c, 5, "soft")
    with pytest.raises(ValueError):
        pfsp_weights_reference(c, 5, "hard", 0)


def test_pfsp_weight_falls_as_the_win_rate_rises():
    games = 200
    for k in (1, 2, 3):
        w = pfsp_weights_reference(_books([games] * 16, np.arange(16) * 13, [0] * 16), 16, "hard", k, 1).astype(np.int64)
        assert (np.diff(w) <= 0).all() and w[0] > w[-1] >= 1, (k, w)
        d = pfsp_weights_reference(_books([games] * 16, [50] * 16, np.arange(16) * 6), 16, "hard", k, 1).astype(np.int64)
        assert (np.diff(d) <= 0).all() and d[0] > d[-1]  # draws count half a win
    v = pfsp_weights_reference(_books([games] * 16, np.arange(16) * 13, [0] * 16), 16, "variance").astype(np.int64)
    assert v.argmax() in (7, 8) and v[0] < v[7] > v[15]  # the even opponents weigh most


def test_pfsp_floor_zero_and_an_always_beaten_agent_give_weight_zero():
    c = _books([10 ** 6, 0], [10 ** 6, 0], [0, 0])
    for k in (1, 2, 3):
        assert pfsp_weights_reference(c, 2, "hard", k, 0)[:3].tolist() == [0, 65535 >> k, 0]
        assert pfsp_weights_reference(c, 2, "hard", k, 1)[0] == 1
    assert pfsp_weights_reference(c, 2, "variance", 2, 0)[0] == 0
    # such a table still draws: the beaten agent is out, the other one takes every env
    assert set(ledger_draw_reference(0, np.arange(1000), 0, pfsp_weights_reference(c, 2, "hard", 2, 0)[:2]).tolist()) == {1}

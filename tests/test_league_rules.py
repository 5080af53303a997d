"""The league's draw rule (include/crl.h "league draws"), restated in plain numpy here -- tests/test_hip_league.py compares the kernels
with THIS restatement -- and the agreement of header, ctypes binding and package for the new entry points.  No GPU."""
import ast
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from competitive_rl_amd import _native as N
from competitive_rl_amd.league import LeagueEnvWrapper, _light_weights, league_draw_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAIN_OPPONENT, DOMAIN_ACTION, DOMAIN_SERVE = 0x4C47554F, 0x4C475541, 0x504F4E47
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (Salmon et al. 2011, the round of csrc/pong_device.h)."""
    c = [np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def league_draw(seed, gid, n, domain, m):
    """value = (word 0 * m) >> 32 of counter (gid lo, gid hi, n, domain), key (seed lo, seed hi)."""
    gid, n = np.asarray(gid, np.uint64), np.asarray(n, np.uint64)
    gid, n = np.broadcast_arrays(gid, n)
    x = philox4x32_10(gid & M32, gid >> np.uint64(32), n, np.full(gid.shape, domain, np.uint64), int(seed) & 0xFFFFFFFF, int(seed) >> 32)[0]
    return ((x * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def test_philox_known_answers():
    """The generator itself: the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors)."""
    z = np.zeros(1, np.uint64)
    assert [int(w[0]) for w in philox4x32_10(z, z, z, z, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = np.full(1, 0xFFFFFFFF, np.uint64)
    assert [int(w[0]) for w in philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    pi = [np.full(1, v, np.uint64) for v in (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)]
    assert [int(w[0]) for w in philox4x32_10(*pi, 0xA4093822, 0x299F31D0)] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


# 99.9 % quantiles of the chi-square distribution with m - 1 degrees of freedom (standard tables): a correct uniform draw exceeds
# them once in a thousand seeds; the seeds below are fixed
CHI2_999 = {2: 10.828, 3: 13.816, 4: 16.266, 5: 18.467, 7: 22.458}


@pytest.mark.parametrize("m,domain", [(4, DOMAIN_OPPONENT), (3, DOMAIN_ACTION), (2, DOMAIN_OPPONENT), (5, DOMAIN_OPPONENT), (7, DOMAIN_OPPONENT)])
def test_draws_are_uniform_over_the_pool(m, domain):
    """2^20 draws: over envs at one counter value, and over the counter for a handful of envs."""
    n = 1 << 20
    for v in (league_draw(12345, np.arange(n), 0, domain, m),
              league_draw(7, np.arange(16)[:, None], np.arange(n // 16)[None, :], domain, m).reshape(-1)):
        assert v.min() >= 0 and v.max() < m
        obs = np.bincount(v, minlength=m).astype(np.float64)
        chi2 = ((obs - n / m) ** 2 / (n / m)).sum()
        assert chi2 < CHI2_999[m], (m, chi2)


def test_opponent_and_action_streams_are_distinct_and_apart_from_the_serves():
    """"opponent of episode e" and "RANDOM's action of step t" of one env are independent streams (domain word), neither is the serve
    sampler's, and seeds / envs / counters all move the draw: agreement between any two is what chance gives for 3 values (1/3)."""
    g, n = np.arange(4096)[:, None], np.arange(64)[None, :]
    opp, act = league_draw(5, g, n, DOMAIN_OPPONENT, 3), league_draw(5, g, n, DOMAIN_ACTION, 3)
    serve = league_draw(5, g, n, DOMAIN_SERVE, 3)
    assert len({DOMAIN_OPPONENT, DOMAIN_ACTION, DOMAIN_SERVE}) == 3
    pairs = {"opp/act": (opp, act), "opp/serve": (opp, serve), "act/serve": (act, serve), "seed": (opp, league_draw(6, g, n, DOMAIN_OPPONENT, 3)),
             "next counter": (opp[:, 1:], opp[:, :-1]), "next env": (opp[1:], opp[:-1]), "high seed word": (opp, league_draw(5 + (1 << 32), g, n, DOMAIN_OPPONENT, 3)),
             "high id word": (opp, league_draw(5, g + (1 << 32), n, DOMAIN_OPPONENT, 3))}
    for what, (a, b) in pairs.items():
        same = float((a == b).mean())  # binomial(262 144, 1/3): sigma = 0.00092; 5 sigma
        assert abs(same - 1 / 3) < 0.005, (what, same)


def test_draws_do_not_depend_on_how_the_id_range_is_cut():
    n, ctr = 1000, np.arange(1000) % 7
    whole = league_draw(3, np.arange(n), ctr, DOMAIN_OPPONENT, 4)
    for cut in (1, 500, 333, 999):
        lo = league_draw(3, 0 + np.arange(cut), ctr[:cut], DOMAIN_OPPONENT, 4)          # shard with env_id_base 0
        hi = league_draw(3, cut + np.arange(n - cut), ctr[cut:], DOMAIN_OPPONENT, 4)    # shard with env_id_base cut
        assert np.array_equal(np.concatenate([lo, hi]), whole)


def test_package_restatement_agrees():
    rs = np.random.RandomState(0)
    gid, ctr = rs.randint(0, 1 << 40, 5000), rs.randint(0, 1 << 31, 5000)
    for seed in (0, 9, (1 << 63) + 12345):
        for domain, m in ((DOMAIN_OPPONENT, 4), (DOMAIN_ACTION, 3)):
            assert np.array_equal(league_draw_reference(seed, gid, ctr, domain, m), league_draw(seed, gid, ctr, domain, m))


def test_header_binding_and_package_agree_on_the_league():
    hdr = open(os.path.join(ROOT, "include", "crl.h")).read()
    defs = dict(re.findall(r"#define (CRL_LEAGUE_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)", hdr))
    assert int(defs["CRL_LEAGUE_MAX_AGENTS"], 0) == N.CRL_LEAGUE_MAX_AGENTS
    assert int(defs["CRL_LEAGUE_DOMAIN_OPPONENT"], 0) == N.CRL_LEAGUE_DOMAIN_OPPONENT == DOMAIN_OPPONENT
    assert int(defs["CRL_LEAGUE_DOMAIN_ACTION"], 0) == N.CRL_LEAGUE_DOMAIN_ACTION == DOMAIN_ACTION
    kinds = re.search(r"enum crl_league_kind \{([^}]*)\}", hdr).group(1)
    assert [tuple(x.strip().split(" = ")) for x in kinds.split(",")] == [("CRL_LEAGUE_RANDOM", "0"), ("CRL_LEAGUE_RULE_BASED", "1"), ("CRL_LEAGUE_LIGHT", "2")]
    assert (N.CRL_LEAGUE_RANDOM, N.CRL_LEAGUE_RULE_BASED, N.CRL_LEAGUE_LIGHT) == (0, 1, 2)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(crl_league_[a-z_0-9]+)\s*\(", code)))
    assert len(declared) == 13 and declared == sorted(s for s in N.SYMBOLS if s.startswith("crl_league_"))
    # the serve sampler's domain word is where the header says, so the three streams cannot meet
    dev = open(os.path.join(ROOT, "competitive_rl_amd", "csrc", "pong_device.h")).read()
    assert "0x504F4E47u" in dev and "0x504F4E47" in hdr
    L = N.load()
    for s in declared:
        assert hasattr(L, s), s
    assert L.crl_league_create(0, 0, 0, 0, None) == -1 and b"crl_league_create" in L.crl_last_error()
    assert L.crl_league_act(None, None, 0, None, 0, None, None) == -1 and L.crl_league_resample(None, None, None) == -1


def test_the_league_refuses_the_full_size_network_and_malformed_weights():
    import competitive_rl_amd as crl

    assert crl.LeagueEnvWrapper is LeagueEnvWrapper
    full = {"conv1_w": np.zeros((16, 4, 4, 4), np.float32), "conv3_w": np.zeros((256, 32, 11, 11), np.float32)}
    with pytest.raises(ValueError, match="full-size ActorCritic is not"):
        _light_weights("MINE", full)
    from competitive_rl_amd.policy_serving import BUILTIN_CHECKPOINTS, load_light_weights

    w = load_light_weights(BUILTIN_CHECKPOINTS["WEAK"])
    assert _light_weights("W", BUILTIN_CHECKPOINTS["WEAK"])["actor_w"].shape == (3, 1600) and _light_weights("W", w)["conv1_w"].dtype == np.float32
    bad = dict(w, conv2_w=np.zeros((16, 16, 3, 3), np.float32))
    with pytest.raises(ValueError, match="conv2_w"):
        _light_weights("W", bad)
    with pytest.raises(TypeError):
        _light_weights("W", 3)

    class NoDevice:
        pass

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LeagueEnvWrapper(NoDevice(), 4)


_MODULES = ("ledger", "arena", "league", "policy_serving")


def test_the_league_modules_import_in_any_order():
    """Each of the 24 orders in an interpreter of its own (eight at a time): no module needs another to have been imported first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    orders = list(itertools.permutations(_MODULES))
    for k in range(0, len(orders), 8):
        procs = [(o, subprocess.Popen([sys.executable, "-c", "; ".join(f"import competitive_rl_amd.{m}" for m in o)], cwd=root,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for o in orders[k:k + 8]]
        for o, p in procs:
            out, _ = p.communicate()
            assert p.returncode == 0, (o, out[-2000:])


@pytest.mark.parametrize("module", ["league", "policy_serving"])
def test_no_import_statement_inside_a_function(module):
    """league.py took LeagueLedger and policy_serving.py took check_sampling through imports inside a function, around an import cycle;
    the rules now live in a leaf module (rules.py) and every import is at the top."""
    path = os.path.join(os.path.dirname(N.__file__), module + ".py")
    tree = ast.parse(open(path).read())
    inside = [(f.name, n.lineno) for f in ast.walk(tree) if isinstance(f, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda))
              for n in ast.walk(f) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not inside, inside

"""Full-size ActorCritic agents in a pool (include/crl.h "full-size agents"): the agreement of header, ctypes binding and library on the
new kind and entry point, the league's own surface left as it was, and the weight check of ``add_full_agent``.  No GPU."""
import os
import re

import numpy as np
import pytest

from competitive_rl_amd import _native as N
from competitive_rl_amd.league import _full_weights, _light_weights
from competitive_rl_amd.policy_serving import BUILTIN_CHECKPOINTS, load_light_weights
from tests.policy_full_weights import make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAGUE_SURFACE = sorted(["crl_league_act", "crl_league_add_builtin", "crl_league_add_light", "crl_league_create", "crl_league_destroy",
                  "crl_league_get_assignment", "crl_league_get_lists", "crl_league_get_stack", "crl_league_reset", "crl_league_resample",
                  "crl_league_seed", "crl_league_set_assignment", "crl_league_set_stack"])


def test_header_binding_and_library_agree_on_the_full_size_kind():
    hdr = open(os.path.join(ROOT, "include", "crl.h")).read()
    assert re.search(r"^#define CRL_POOL_KIND_FULL 3\b", hdr, flags=re.M) and N.CRL_POOL_KIND_FULL == 3
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+crl_pool_add_full\s*\(\s*crl_league\s*\*", code)
    assert "crl_pool_add_full" in N.SYMBOLS and len(N.SIGNATURES["crl_pool_add_full"][1]) == 10
    assert hasattr(N.load(), "crl_pool_add_full")
    # the enum and the league's thirteen entry points are what they were
    kinds = re.search(r"enum crl_league_kind \{([^}]*)\}", hdr).group(1)
    assert [x.strip() for x in kinds.split(",")] == ["CRL_LEAGUE_RANDOM = 0", "CRL_LEAGUE_RULE_BASED = 1", "CRL_LEAGUE_LIGHT = 2"]
    assert sorted(set(re.findall(r"\b(crl_league_[a-z_0-9]+)\s*\(", code))) == LEAGUE_SURFACE
    assert sorted(s for s in N.SYMBOLS if s.startswith("crl_league_")) == LEAGUE_SURFACE
    assert N.CRL_POOL_KIND_FULL not in (N.CRL_LEAGUE_RANDOM, N.CRL_LEAGUE_RULE_BASED, N.CRL_LEAGUE_LIGHT)


def test_the_entry_point_refuses_null_arguments_before_any_gpu_call():
    L = N.load()
    w = make_weights(5)
    ptr = [np.ascontiguousarray(w[k], np.float32).ctypes.data for k in
           ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "actor_w", "actor_b")]
    for args in ([None] * 8 + [0], ptr + [0], ptr + [-4], [None] * 8 + [64]):
        assert L.crl_pool_add_full(None, *args) == -1
        assert b"crl_pool_add_full" in L.crl_last_error()


def test_full_weights_accepts_full_size_sets_and_refuses_the_rest():
    w = make_weights(5)  # (carries critic_w / critic_b beside the eight arrays: they are ignored)
    assert "critic_w" in w
    got = _full_weights("BIG", w)
    assert sorted(got) == sorted(k for k in w if not k.startswith("critic")) and got["conv3_w"].shape == (256, 32, 11, 11)
    assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] for v in got.values()) and np.array_equal(got["actor_w"], w["actor_w"])
    eight = {k: v.astype(np.float64) for k, v in w.items() if not k.startswith("critic")}
    assert _full_weights("BIG", eight)["conv2_w"].dtype == np.float32
    weak = load_light_weights(BUILTIN_CHECKPOINTS["WEAK"])
    with pytest.raises(ValueError, match="add_agent"):
        _full_weights("W", weak)
    with pytest.raises(ValueError, match="conv3_w"):
        _full_weights("BIG", dict(w, conv3_w=np.zeros((256, 32, 10, 10), np.float32)))
    with pytest.raises(ValueError, match="actor_b"):
        _full_weights("BIG", {k: v for k, v in w.items() if k != "actor_b"})
    with pytest.raises(TypeError, match="BIG"):
        _full_weights("BIG", 3)


def test_light_weights_still_refuses_the_full_size_network_with_the_old_words():
    with pytest.raises(ValueError, match="full-size ActorCritic is not"):
        _light_weights("MINE", make_weights(5))
    with pytest.raises(ValueError, match="add_full_agent"):
        _light_weights("MINE", make_weights(5))

"""The arena's pair draw and its balance weights (include/crl.h "arena draws", "balance weights"), restated in plain numpy here --
tests/test_hip_arena.py compares the kernels with the package's restatements, this file compares those with THIS one and with answers
worked out by hand -- and the agreement of header, ctypes binding and library for the crl_arena_* entry points.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from competitive_rl_amd import _native as N
from competitive_rl_amd.arena import ArenaBooks, LeagueArena, arena_draw_reference, balance_weights_reference, payoff_from_counters
from competitive_rl_amd.league import league_draw_reference
from tests.test_league_rules import DOMAIN_ACTION, DOMAIN_OPPONENT, DOMAIN_SERVE, M32, philox4x32_10
from tests.test_ledger_rules import DOMAIN_LEDGER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAIN_PAIR = 0x4C475550  # "LGUP"
W4 = [[0, 3, 1, 0], [2, 0, 0, 5], [1, 1, 0, 0], [0, 4, 2, 0]]  # a non-uniform table with zero cells, [left][right]


def pair_draw(seed, gid, n, w):
    """r = (word 0 * T) >> 32 of counter (gid lo, gid hi, n, "LGUP"), key (seed lo, seed hi); the first cell, rows first and the columns
    of a row inside, whose cumulative weight exceeds r, found by walking the table.  Returns the cell as (left, right)."""
    gid, n = np.broadcast_arrays(np.asarray(gid, np.uint64), np.asarray(n, np.uint64))
    x = philox4x32_10(gid & M32, gid >> np.uint64(32), n, np.full(gid.shape, DOMAIN_PAIR, np.uint64), int(seed) & 0xFFFFFFFF, int(seed) >> 32)[0]
    total = sum(int(v) for row in w for v in row)
    assert 0 < total < 2 ** 32
    r = (x * np.uint64(total)) >> np.uint64(32)
    left, right, cum = np.full(gid.shape, -1, np.int64), np.full(gid.shape, -1, np.int64), 0
    for a, row in enumerate(w):
        for b, v in enumerate(row):
            cum += int(v)
            hit = (left < 0) & (r < np.uint64(cum))
            left[hit], right[hit] = a, b
    return left, right


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_header_binding_and_library_agree_on_the_arena():
    hdr = open(os.path.join(ROOT, "include", "crl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(crl_arena_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(s for s in N.SYMBOLS if s.startswith("crl_arena_"))
    for want in ("create", "destroy", "seed", "reset", "set_agents", "set_weights", "get_weights", "balance_weights", "get_counters",
                 "set_counters", "get_env_state", "set_env_state", "step"):
        assert "crl_arena_" + want in declared, want
    L = N.load()
    for s in declared:
        assert hasattr(L, s), s
    defs = dict(re.findall(r"#define (CRL_ARENA_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)", hdr))
    assert int(defs["CRL_ARENA_DOMAIN_PAIR"], 0) == N.CRL_ARENA_DOMAIN_PAIR == DOMAIN_PAIR
    assert len({DOMAIN_PAIR, DOMAIN_LEDGER, DOMAIN_OPPONENT, DOMAIN_ACTION, DOMAIN_SERVE}) == 5
    assert int(defs["CRL_ARENA_COUNTERS"]) == N.CRL_ARENA_COUNTERS == len(N.CRL_ARENA_COUNTER_NAMES) == 6
    order = re.search(r"enum crl_arena_counter \{([^}]*)\}", hdr).group(1)
    assert [x.strip().split(" = ")[0][len("CRL_ARENA_"):].lower() for x in order.split(",")] == list(N.CRL_ARENA_COUNTER_NAMES)


def test_arena_entry_points_refuse_null_and_bad_arguments():
    L = N.load()
    h = ctypes.c_void_p()
    assert L.crl_arena_create(0, 8, 0, 0, 4, None) == -1 and b"crl_arena_create" in L.crl_last_error()
    for envs, base, agents in ((0, 0, 4), (-3, 0, 4), (1 << 30, 0, 4), (8, -1, 4), (8, 0, 0), (8, 0, 17)):
        assert L.crl_arena_create(0, envs, base, 0, agents, ctypes.byref(h)) == -1 and b"crl_arena_create" in L.crl_last_error()
        assert not h.value
    assert L.crl_arena_step(None, None, None, 0, None, 0, None, None) == -1 and b"crl_arena_step" in L.crl_last_error()
    for name, args in (("seed", (None, 0, None)), ("reset", (None, None)), ("set_agents", (None, 4, None)), ("set_weights", (None, None, 0, None)),
                       ("get_weights", (None, None, None)), ("balance_weights", (None, None, 0, 1, None)), ("get_counters", (None, None, None, None)),
                       ("set_counters", (None, None, None, None)), ("get_env_state", (None, None, None, None, None)),
                       ("set_env_state", (None, None, None, None, None)), ("draw", (None, None, None, None))):
        assert getattr(L, "crl_arena_" + name)(*args) == -1 and b"crl_arena_" + name.encode() in L.crl_last_error(), name
    L.crl_arena_destroy(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ArenaBooks(8, 4, "cpu")
    with pytest.raises(ValueError, match="resized_dim=42"):
        LeagueArena(object(), 8)
    import competitive_rl_amd as crl

    assert crl.LeagueArena is LeagueArena and crl.arena_draw_reference is arena_draw_reference
    assert crl.balance_weights_reference is balance_weights_reference


def test_a_one_hot_table_always_draws_its_cell():
    rs = np.random.RandomState(1)
    gid, ctr = rs.randint(0, 1 << 40, 2000), rs.randint(0, 1 << 31, 2000)
    for a, (l, r), weight in ((4, (2, 1), 1), (16, (15, 0), 7), (1, (0, 0), 0xFFFFFFFF), (5, (0, 4), 65536)):
        w = np.zeros((a, a), np.int64)
        w[l, r] = weight
        left, right = arena_draw_reference(9, gid, ctr, w)
        assert (left == l).all() and (right == r).all()


def test_a_zero_weight_cell_is_never_drawn():
    n = 100_000
    for w in (W4, [[0, 1], [1000, 0]], np.eye(6, dtype=np.int64)[::-1].tolist()):
        w = np.asarray(w)
        by_gid, by_ctr = arena_draw_reference(21, np.arange(n), 0, w), arena_draw_reference(22, 5, np.arange(n), w)
        seen = np.zeros_like(w)
        for left, right in (by_gid, by_ctr):
            np.add.at(seen, (left, right), 1)
        assert ((seen == 0) == (w == 0)).all(), (w, seen)


def test_scaling_the_table_leaves_every_draw_unchanged():
    """(x * kT) >> 32 lies in [k * c, k * (c + 1)) exactly when (x * T) >> 32 is c less a fraction: floor(x k T / 2^32) < k * cum holds
    if and only if floor(x T / 2^32) < cum, for integers k, cum."""
    rs = np.random.RandomState(2)
    gid, ctr = rs.randint(0, 1 << 40, 5000), rs.randint(0, 1 << 31, 5000)
    w = np.asarray(W4, np.int64)
    base = arena_draw_reference(3, gid, ctr, w)
    for k in (2, 3, 1000, 65535, (2 ** 32 - 1) // int(w.sum())):
        assert _same(arena_draw_reference(3, gid, ctr, w * k), base), k


def test_the_order_of_the_cells_is_row_major():
    """Two cells of weight 1: r is 0 or 1, and 0 must go to the cell that comes first with rows before columns.  With unit weights the
    cell is the uniform draw over a * a values under the arena's domain word."""
    rs = np.random.RandomState(3)
    gid, ctr = rs.randint(0, 1 << 40, 3000), rs.randint(0, 1 << 31, 3000)
    w = np.zeros((4, 4), np.int64)
    w[0, 3] = w[1, 0] = 1  # (0, 3) is cell 3, (1, 0) is cell 4: row-major puts (0, 3) first, column-major (1, 0)
    half = league_draw_reference(5, gid, ctr, DOMAIN_PAIR, 2)
    left, right = arena_draw_reference(5, gid, ctr, w)
    assert np.array_equal(left, half) and np.array_equal(right, np.where(half == 0, 3, 0)) and 0 < half.sum() < len(half)
    for a in (1, 3, 16):
        cell = league_draw_reference(6, gid, ctr, DOMAIN_PAIR, a * a)
        left, right = arena_draw_reference(6, gid, ctr, np.ones((a, a), np.int64))
        assert np.array_equal(left, cell // a) and np.array_equal(right, cell % a)
        assert a == 1 or not np.array_equal(cell, league_draw_reference(6, gid, ctr, DOMAIN_LEDGER, a * a))
    for seed, w in ((3, W4), ((1 << 63) + 9, rs.randint(0, 1000, (16, 16))), (8, [[0x7FFFFFFF, 0], [0x7FFFFFFF, 1]])):
        assert _same(arena_draw_reference(seed, gid, ctr, w), pair_draw(seed, gid, ctr, np.asarray(w).tolist()))


def test_known_answers():
    """Computed once from league_draw_reference under the domain word "LGUP" and a walk of W4's sixteen cells."""
    left, right = arena_draw_reference(12345, np.arange(8), 0, W4)
    assert left.tolist() == [1, 0, 3, 0, 3, 3, 0, 3] and right.tolist() == [3, 1, 1, 2, 1, 2, 1, 1]
    left, right = arena_draw_reference((1 << 63) + 9, (1 << 40) + np.arange(6), np.arange(6) * 1000003, W4)
    assert left.tolist() == [3, 0, 3, 2, 0, 0] and right.tolist() == [1, 2, 1, 0, 2, 1]
    left, right = arena_draw_reference(7, 3, np.arange(8), [[0, 1], [1, 0]])
    assert left.tolist() == [1, 0, 0, 0, 0, 1, 1, 0] and right.tolist() == [0, 1, 1, 1, 1, 0, 0, 1]
    assert _same(pair_draw(12345, np.arange(8), 0, W4), ([1, 0, 3, 0, 3, 3, 0, 3], [3, 1, 1, 2, 1, 2, 1, 1]))


def test_a_table_that_sums_to_zero_or_past_2_32_is_rejected():
    for bad in (np.zeros((3, 3), np.int64), [[0xFFFFFFFF, 1], [0, 0]], [[1 << 31, 1 << 31], [0, 0]], [[1, 2, 3]], [1, 2], np.ones((17, 17), np.int64),
                [[-1, 2], [3, 4]]):
        with pytest.raises(ValueError):
            arena_draw_reference(0, 0, 0, bad)
    assert arena_draw_reference(0, 0, 0, [[0xFFFFFFFF, 0], [0, 0]])[0] == 0


def test_draws_do_not_depend_on_how_the_id_range_is_cut():
    n, ctr = 1003, np.arange(1003) % 5
    whole = arena_draw_reference(3, np.arange(n), ctr, W4)
    for cut in (1, 500, 999):
        lo, hi = arena_draw_reference(3, np.arange(cut), ctr[:cut], W4), arena_draw_reference(3, cut + np.arange(n - cut), ctr[cut:], W4)
        assert _same((np.concatenate([lo[0], hi[0]]), np.concatenate([lo[1], hi[1]])), whole)


def _books(episodes):
    c = np.zeros((N.CRL_ARENA_COUNTERS, 16, 16), np.int64)
    e = np.asarray(episodes, np.int64)
    c[0, :e.shape[0], :e.shape[1]] = e
    c[1:] = 12345  # only the episodes are read
    return c


def test_balance_weights_of_an_empty_book_are_the_floor_on_every_scheduled_cell():
    for agents in (1, 2, 4, 16):
        for mirror in (False, True):
            for floor in (1, 7, 0):
                w = balance_weights_reference(_books(np.zeros((16, 16))), agents, mirror, floor)
                sched = np.zeros((16, 16), bool)
                sched[:agents, :agents] = True
                if not mirror:
                    sched &= ~np.eye(16, dtype=bool)
                assert w.dtype == np.uint32 and w.shape == (16, 16) and (w[sched] == floor).all() and (w[~sched] == 0).all()


def test_balance_weights_with_one_pair_ahead():
    """By hand, 3 agents: cell (0, 1) has 10 episodes, (1, 0) has 4, every other scheduled cell none -> m = 10, weights floor + 10 - e."""
    e = np.zeros((3, 3))
    e[0, 1], e[1, 0] = 10, 4
    e[2, 2] = 50  # a mirror match that is not scheduled must not move m
    w = balance_weights_reference(_books(e), 3, False, 1)
    assert w[:4, :4].tolist() == [[0, 1, 11, 0], [7, 0, 11, 0], [11, 11, 0, 0], [0, 0, 0, 0]] and w.sum() == 52
    w = balance_weights_reference(_books(e), 3, True, 1)  # scheduled now: m = 50
    assert w[:4, :4].tolist() == [[51, 41, 51, 0], [47, 51, 51, 0], [51, 51, 1, 0], [0, 0, 0, 0]]
    w = balance_weights_reference(_books(e), 2, False, 0)  # agent 2 is outside the pool; floor 0 takes the leading pair out
    assert w[:3, :3].tolist() == [[0, 0, 0], [6, 0, 0], [0, 0, 0]]
    # episodes beyond the pool are not looked at
    far = _books(e)
    far[0, 5, 6] = 10 ** 12
    assert np.array_equal(balance_weights_reference(far, 3, False, 1), balance_weights_reference(_books(e), 3, False, 1))


def test_balance_weights_cap_at_65535():
    e = np.zeros((4, 4))
    e[0, 1], e[0, 2], e[0, 3] = 10 ** 12, 10 ** 12 - 65534, 10 ** 12 - 65536
    w = balance_weights_reference(_books(e), 4, False, 3)
    assert w[0, :4].tolist() == [0, 3, 3 + 65534, 3 + 65535] and (w[1:4, :4][~np.eye(4, dtype=bool)[1:]] == 3 + 65535).all()
    # the largest table the device call accepts still sums below 2^32
    assert 256 * (2 ** 24 - 65536 + 65535) < 2 ** 32
    # pairs played less weigh more, and such a table draws them more often
    e = np.arange(16).reshape(4, 4) * 100
    w = balance_weights_reference(_books(e), 4, False, 1)[:4, :4].astype(np.int64)
    off = ~np.eye(4, dtype=bool)
    assert (np.diff(w[off]) < 0).all()
    left, right = arena_draw_reference(4, np.arange(50_000), 0, w)
    seen = np.zeros((4, 4), np.int64)
    np.add.at(seen, (left, right), 1)
    assert seen[0, 1] > seen[1, 2] > seen[3, 2] > 0 and not np.diag(seen).any()


def test_payoff_is_antisymmetric_over_the_seats_and_nan_where_nothing_was_played():
    rs = np.random.RandomState(0)
    for _ in range(300):
        lw, rw, d = rs.randint(0, 50, (5, 5)), rs.randint(0, 50, (5, 5)), rs.randint(0, 5, (5, 5))
        lw[0, 1] = rw[0, 1] = d[0, 1] = lw[1, 0] = rw[1, 0] = d[1, 0] = 0  # a pair never played in either seat order
        lw[2, 2] = rw[2, 2] = d[2, 2] = 0
        e = lw + rw + d
        p = payoff_from_counters(dict(episodes=e, left_wins=lw, right_wins=rw, draws=d, return_sum=lw - rw, length_sum=e * 7))
        s, played = p["score"], (e + e.T) > 0
        assert np.isnan(s[0, 1]) and np.isnan(s[1, 0]) and np.isnan(s[2, 2]) and np.isnan(p["win_rate"][0, 1]) and not np.isnan(s[played]).any()
        assert ((s + s.T)[played] == 1).all()
        by_hand = (lw + rw.T + (d + d.T) / 2)[played] / (e + e.T)[played]  # a's wins and half the draws against b, both seat orders
        assert np.allclose(s[played], by_hand, rtol=0, atol=1e-15)
        assert np.array_equal(p["mean_length"][e > 0], np.full(int((e > 0).sum()), 7.0))
        assert np.allclose(p["win_rate"][e > 0], ((lw + d / 2) / np.maximum(e, 1))[e > 0], rtol=0, atol=1e-15)

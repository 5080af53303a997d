"""The numpy restatement of include/crl.h "car league" alone (rules.car_league_reference, car_league_draw_reference, car_league_q):
what the device tests replay against is itself pinned here, without a GPU."""
import numpy as np
import pytest

from competitive_rl_amd import _native as N
from competitive_rl_amd import rules as R

A = N.CRL_LEAGUE_MAX_AGENTS


def sequence(seed, steps, n, p_done=0.3):
    rs = np.random.RandomState(seed)
    rewards = (rs.standard_normal((steps, n, 2)) * 3).astype(np.float32)
    dones = (rs.random_sample((steps, n)) < p_done).astype(np.uint8)
    return rewards, dones


def test_weight_zero_agents_are_never_drawn_and_every_other_one_is():
    w = np.array([30, 0, 10, 0, 700, 20], np.uint32)
    gid, ctr = np.meshgrid(np.arange(400, dtype=np.uint64), np.arange(8, dtype=np.uint64), indexing="ij")
    drawn = R.car_league_draw_reference(11, gid, ctr, w)
    assert drawn.shape == gid.shape and set(np.unique(drawn)) == {0, 2, 4, 5}
    # the heavy agent takes about its share, 700 / 760 = 0.92
    assert 0.89 < (drawn == 4).mean() < 0.95


def test_a_pool_of_one_always_draws_it_whatever_its_weight():
    for w in ([1], [0xFFFFFFFF], [5]):
        assert (R.car_league_draw_reference(3, np.arange(100), 7, np.array(w, np.uint64)) == 0).all()
    with pytest.raises(ValueError):
        R.car_league_draw_reference(3, 0, 0, [0, 0])
    with pytest.raises(ValueError):
        R.car_league_draw_reference(3, 0, 0, [0xFFFFFFFF, 1])


def test_a_draw_depends_on_seed_gid_counter_and_table_alone():
    w = np.array([5, 1, 9, 2], np.uint32)
    gid = np.arange(64, dtype=np.uint64)
    whole = R.car_league_draw_reference(21, gid, 3, w)
    # one env at a time, any order, padded tables: the same draws
    assert [int(R.car_league_draw_reference(21, int(g), 3, w)) for g in gid[::-1]] == whole[::-1].tolist()
    assert (R.car_league_draw_reference(21, gid, 3, np.concatenate([w, np.zeros(12, np.uint32)])) == whole).all()
    # a shard's global ids: envs [40, 64) of the batch
    assert (R.car_league_draw_reference(21, np.arange(24, dtype=np.uint64) + np.uint64(40), 3, w) == whole[40:]).all()
    # ... and every one of the four matters
    for other in (R.car_league_draw_reference(22, gid, 3, w), R.car_league_draw_reference(21, gid + np.uint64(64), 3, w),
                  R.car_league_draw_reference(21, gid, 4, w), R.car_league_draw_reference(21, gid, 3, w[::-1].copy())):
        assert (other != whole).any()
    # its own domain: not the ledger's draws
    assert (R.league_draw_reference(21, gid, 3, N.CRL_LEDGER_DOMAIN_OPPONENT, 17) != R.league_draw_reference(21, gid, 3, N.CRL_CAR_LEAGUE_DOMAIN, 17)).any()
    assert N.CRL_CAR_LEAGUE_DOMAIN not in (N.CRL_LEDGER_DOMAIN_OPPONENT, N.CRL_LEAGUE_DOMAIN_OPPONENT, N.CRL_ARENA_DOMAIN_PAIR,
                                           N.CRL_CAR_DRIVER_DOMAIN, N.CRL_CAR_DRIVER_DOMAIN + 1, N.CRL_CAR_POLICY_DOMAIN, N.CRL_CAR_POLICY_DOMAIN + 1)


def test_the_shared_draw_under_each_domain_is_what_the_two_named_references_return():
    from competitive_rl_amd.ledger import ledger_draw_reference

    w = np.array([7, 0, 3, 900, 1, 0, 0, 40, 2, 2, 65535, 1, 9, 0, 5, 11], np.uint32)  # 16 weights, zeros among them
    gid = np.uint64(2 ** 32) + np.arange(300, dtype=np.uint64) * np.uint64(0x1_0000_0007)  # above 2^32: the counter's second word counts
    ctr = np.arange(300, dtype=np.uint64) % np.uint64(5)
    ledger, car = ledger_draw_reference(9, gid, ctr, w), R.car_league_draw_reference(9, gid, ctr, w)
    assert (R.weighted_draw_reference(9, gid, ctr, N.CRL_LEDGER_DOMAIN_OPPONENT, w) == ledger).all()
    assert (R.weighted_draw_reference(9, gid, ctr, N.CRL_CAR_LEAGUE_DOMAIN, w) == car).all()
    assert (ledger != car).any() and not set(np.unique(np.concatenate([ledger, car]))) & {1, 5, 6, 13}
    # the high word of gid reaches the draw
    assert (R.weighted_draw_reference(9, gid - np.uint64(2 ** 32), ctr, N.CRL_CAR_LEAGUE_DOMAIN, w) != car).any()


def test_q_rounds_to_nearest_even_in_units_of_1_256_and_books_zero_for_non_finite_returns():
    x = np.array([0.0, 1.0, -1.0, 1.5 / 256, 2.5 / 256, -0.5 / 256, 900.25, np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    assert R.car_league_q(x).tolist() == [0, 256, -256, 2, 2, 0, 230464, 0, 0, 0, 2 ** 62, -2 ** 62]


def test_nan_returns_book_a_draw_and_zero_in_the_sums():
    st = R.car_league_state(4)
    st["agent"][:] = [0, 1, 0, 1]
    rewards = np.zeros((2, 4, 2), np.float32)
    rewards[0, 0] = [np.nan, 1.0]   # NaN on car 0's side
    rewards[0, 1] = [2.0, np.nan]   # ... on car 1's
    rewards[0, 2] = [np.inf, 1.0]   # inf > 1: a win, but q books 0
    rewards[0, 3] = [1.0, 1.0]      # equal: a draw
    dones = np.array([[0, 0, 0, 0], [1, 1, 1, 1]], np.uint8)
    out, after = R.car_league_reference(st, rewards, dones, 2, [1, 1], seed=0, redraw=False)
    c = dict(zip(R.CAR_LEAGUE_COUNTER_NAMES, out["counters"]))
    assert c["episodes"][:2].tolist() == [2, 2] and c["wins"][:2].tolist() == [1, 0] and c["losses"][:2].tolist() == [0, 0]
    assert c["draws"][:2].tolist() == [1, 2]
    assert c["return_sum"][:2].tolist() == [0, 2 * 256 + 256] and c["opponent_return_sum"][:2].tolist() == [256 + 256, 256]
    assert c["length_sum"][:2].tolist() == [4, 4]
    assert (after == st["agent"]).all() and (out["draw_ctr"] == 0).all()       # redraw=False keeps both
    assert not out["ret"].any() and not out["len"].any()                       # (NaN included: the episode's sums start over)


def test_quantised_sums_equal_a_python_integer_recomputation():
    steps, n, agents = 40, 37, 5
    rewards, dones = sequence(5, steps, n)
    w = [4, 0, 1, 9, 2]
    st = R.car_league_draw_all_reference(R.car_league_state(n), agents, w, seed=9, env_id_base=100)
    assert (st["draw_ctr"] == 1).all() and set(np.unique(st["agent"])) <= {0, 2, 3, 4}
    out, after = R.car_league_reference(st, rewards, dones, agents, w, seed=9, env_id_base=100)
    # the same books kept with Python integers and floats rounded to float32 after every add, one env at a time
    books = {k: [0] * A for k in R.CAR_LEAGUE_COUNTER_NAMES}
    for e in range(n):
        agent, ctr, ret, length = int(st["agent"][e]), 1, [np.float32(0), np.float32(0)], 0
        for t in range(steps):
            ret = [np.float32(ret[c] + rewards[t, e, c]) for c in range(2)]
            length += 1
            if dones[t, e]:
                books["episodes"][agent] += 1
                books["wins" if ret[0] > ret[1] else "losses" if ret[0] < ret[1] else "draws"][agent] += 1
                books["return_sum"][agent] += int(round(float(ret[0]) * 256.0))
                books["opponent_return_sum"][agent] += int(round(float(ret[1]) * 256.0))
                books["length_sum"][agent] += length
                ret, length = [np.float32(0), np.float32(0)], 0
                agent = int(R.car_league_draw_reference(9, 100 + e, ctr, w))
                ctr += 1
            assert after[t, e] == agent
        assert out["draw_ctr"][e] == ctr and out["len"][e] == length and out["ret"][e].tolist() == [float(x) for x in ret]
    for i, k in enumerate(R.CAR_LEAGUE_COUNTER_NAMES):
        assert out["counters"][i].tolist() == books[k], k
    assert out["counters"][0].sum() == int(dones.sum()) and out["counters"][0, 1] == 0
    assert (out["counters"][1] + out["counters"][2] + out["counters"][3] == out["counters"][0]).all()
    assert not st["counters"].any()  # the replay works on copies


def test_a_zero_sum_table_keeps_agent_and_counter():
    rewards, dones = sequence(6, 10, 9)
    st = R.car_league_draw_all_reference(R.car_league_state(9), 3, [1, 1, 1], seed=2)
    out, after = R.car_league_reference(st, rewards, dones, 3, [0, 0, 0], seed=2)
    assert (after == st["agent"]).all() and (out["draw_ctr"] == st["draw_ctr"]).all() and out["counters"][0].sum() == dones.sum()
    # ... and an env that had no draw yet books nothing
    out, _ = R.car_league_reference(R.car_league_state(9), rewards, dones, 3, [0, 0, 0], seed=2)
    assert not out["counters"].any() and (out["agent"] == -1).all()


def test_reset_agent_zeroes_one_column_only():
    rewards, dones = sequence(7, 30, 20)
    st = R.car_league_draw_all_reference(R.car_league_state(20), 4, [1, 2, 3, 4], seed=1)
    out, _ = R.car_league_reference(st, rewards, dones, 4, [1, 2, 3, 4], seed=1)
    assert (out["counters"][0, :4] > 0).all()
    cut = R.car_league_reset_agent_reference(out, 2)
    assert not cut["counters"][:, 2].any()
    keep = [a for a in range(A) if a != 2]
    assert (cut["counters"][:, keep] == out["counters"][:, keep]).all()
    for k in ("agent", "ret", "len", "draw_ctr"):
        assert (cut[k] == out[k]).all()


def test_columns_name_the_slot_in_one_array_and_nobody_in_the_other():
    pool = [("STYLE", 0), ("STYLE", 1), ("NETWORK", 3), (N.CRL_CAR_LEAGUE_NETWORK, 0)]
    net, style = R.car_league_columns(pool, [0, 1, 2, 3, -1, 9])
    assert net.tolist() == [-1, -1, 3, 0, -1, -1] and style.tolist() == [0, 1, -1, -1, -1, -1]
    assert net.dtype == np.int32 and style.dtype == np.int32

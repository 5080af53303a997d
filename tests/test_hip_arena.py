"""LeagueArena / ArenaBooks (competitive_rl_amd/arena.py, csrc/pong_arena.hip) on the device: the per-pair books against a numpy replay
of the steps, the pair redraws against the written rule (restated in tests/test_arena_rules.py), the balance kernel against its numpy
restatement, both seats against crl_policy objects fed the same frames, sharding, checkpoints and the hot loop's freedom from host
work.  Books, draws and weights are integers: tolerance 0; the CNN agents' logits agree to the 1e-4 of tests/test_hip_policy_parity.py."""
import time

import numpy as np
import pytest
import torch

from competitive_rl_amd import _native as N
from competitive_rl_amd.arena import ArenaBooks, LeagueArena, arena_draw_reference, balance_weights_reference
from competitive_rl_amd.league import league_draw_reference
from tests.test_arena_rules import W4, pair_draw
from tests.test_hip_league import _env, _near_the_end, _need_gpu

pytestmark = pytest.mark.gpu

NAMES = N.CRL_ARENA_COUNTER_NAMES
POOL4 = ["RANDOM", "RULE_BASED", "WEAK", "MEDIUM"]


class Replay:
    """The books in numpy: feed it every step's (pairs that played (N, 2), left agent's reward, done)."""

    def __init__(self, n, agents):
        self.agents = agents
        self.ret, self.len = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.c = {k: np.zeros((agents, agents), np.int64) for k in NAMES}
        self.ignored = 0

    def step(self, pairs, reward, done):
        assert np.array_equal(reward, np.round(reward))
        self.ret += reward.astype(np.int64)
        self.len += 1
        d = done.astype(bool)
        ok = d & (pairs >= 0).all(1) & (pairs < self.agents).all(1)
        self.ignored += int((d & ~ok).sum())
        cell, r = (pairs[ok, 0], pairs[ok, 1]), self.ret[ok]
        for k, v in (("episodes", 1), ("left_wins", r > 0), ("right_wins", r < 0), ("draws", r == 0), ("return_sum", r), ("length_sum", self.len[ok])):
            np.add.at(self.c[k], cell, np.asarray(v, np.int64))
        self.ret[d], self.len[d] = 0, 0

    def same_as(self, books, rows=None):
        got = books.counters()
        for k in NAMES:
            assert np.array_equal(got[k], self.c[k]), (k, got[k], self.c[k])
        assert got["ignored"] == self.ignored
        ret, length, _ = (t.cpu().numpy() for t in books.env_state())
        rows = slice(None) if rows is None else rows
        assert np.array_equal(ret[rows], self.ret[rows]) and np.array_equal(length[rows], self.len[rows])


def _made_up(n, agents, steps, seed, lo=-1, hi=None):
    """Made-up steps from a seeded numpy generator: ids in [lo, hi) on either seat (some outside the pool), rewards in {-1, 0, 1} in
    column 0 of an (N, 2) buffer, one done flag in eight."""
    rs = np.random.RandomState(seed)
    hi = agents + 1 if hi is None else hi
    pairs = rs.randint(lo, hi, (steps, n, 2)).astype(np.int32)
    reward = np.full((steps, n, 2), 7.0, np.float32)  # the right agent's column must never be read
    reward[:, :, 0] = rs.randint(-1, 2, (steps, n))
    done = (rs.randint(0, 8, (steps, n)) == 0).astype(np.uint8)
    return pairs, reward, done


def _expect_out(seed, gid, ctr, table, pairs, done, redraw):
    """pairs_out and the draw counters after a step, by the written rule"""
    d = done.astype(bool)
    if not redraw:
        return pairs.copy(), ctr
    left, right = arena_draw_reference(seed, gid, ctr, table)
    out = np.where(d[:, None], np.stack([left, right], 1), pairs).astype(np.int32)
    return out, ctr + d


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1003])
def test_books_equal_a_numpy_replay_of_made_up_steps(n):
    """40 steps at sizes around the wavefront and the block, with a step where EVERY env ends on the same cell, one where the 64 lanes
    of a wavefront end on 64 different cells, one without any end, and ids outside the pool on either seat.  Every second step asks
    for redraws.  A second object takes the pairs in place (pairs_out aliased to pairs) and must show the same."""
    _need_gpu()
    agents, steps, seed, base = 9, 40, 31, (1 << 33) + 5
    table = np.random.RandomState(7).randint(0, 4, (agents, agents))
    pairs, reward, done = _made_up(n, agents, steps, n)
    pairs[5], done[5] = (2, 1), 1                                    # every env ends on cell (2, 1)
    k = np.arange(n) % 64
    pairs[9, :, 0], pairs[9, :, 1], done[9] = k // agents, k % agents, 1  # lane j of every wavefront ends on cell j: 64 different ones
    done[13] = 0                                                     # no end at all
    a, b = (ArenaBooks(n, agents, "cuda:0", seed=seed, env_id_base=base) for _ in range(2))
    a.set_weights(table), b.set_weights(table)
    replay, ctr, gid = Replay(n, agents), np.zeros(n, np.int64), base + np.arange(n)
    for t in range(steps):
        redraw = t % 2 == 1
        p, r, d = torch.from_numpy(pairs[t]).cuda(), torch.from_numpy(reward[t]).cuda(), torch.from_numpy(done[t]).cuda()
        out = a.update(p, r if t % 3 else r[:, 0].contiguous(), d, redraw=redraw)
        same = p.clone()
        assert b.update(same, r, d, redraw=redraw, out=same) is same
        expect, ctr = _expect_out(seed, gid, ctr, table, pairs[t], done[t], redraw)
        assert torch.equal(p.cpu(), torch.from_numpy(pairs[t])), "the pairs passed in were written to"
        assert np.array_equal(out.cpu().numpy(), expect) and np.array_equal(same.cpu().numpy(), expect), t
        replay.step(pairs[t].astype(np.int64), reward[t, :, 0], done[t])
    replay.same_as(a), replay.same_as(b)
    c = a.counters()
    assert c["episodes"][2, 1] >= n and (c["episodes"].reshape(-1)[:min(n, 64)] > 0).all()
    if n >= 63:
        assert c["ignored"] > 0 and c["draws"].sum() > 0 and c["right_wins"].sum() > 0 and (c["return_sum"] != 0).any()
    for x in (a, b):
        assert np.array_equal(x.env_state()[2].cpu().numpy().view(np.uint32), ctr)
    a.reset()
    c = a.counters()
    assert all(not c[k].any() for k in NAMES) and c["ignored"] == 0 and not a.env_state()[0].any() and not a.env_state()[1].any()
    assert np.array_equal(a.env_state()[2].cpu().numpy().view(np.uint32), ctr) and np.array_equal(a.weights(), table)  # reset keeps these
    a.seed(32)
    assert not a.env_state()[2].any()
    fresh = a.draw(torch.from_numpy(pairs[0]).cuda())
    left, right = arena_draw_reference(32, gid, 0, table)
    assert np.array_equal(fresh.cpu().numpy(), np.stack([left, right], 1)) and (a.env_state()[2] == 1).all()
    a.close(), b.close()


def test_every_redraw_follows_the_written_rule():
    """A non-uniform table with zero cells: every redrawn pair is arena_draw_reference at the env's global id and counter (and this
    file's own walk of the table), envs that did not end keep pair and counter, and with a table that sums to 0 nothing moves."""
    _need_gpu()
    n, agents, steps, seed, base = 1003, 4, 60, 77, 1000
    pairs, reward, done = _made_up(n, agents, steps, 3, lo=0, hi=agents)
    books = ArenaBooks(n, agents, "cuda:0", seed=seed, env_id_base=base)
    assert np.array_equal(books.weights(), 1 - np.eye(4, dtype=np.uint32))  # after create: 1 off the diagonal
    books.set_weights(W4)
    cur = torch.from_numpy(pairs[0]).cuda()
    gid, ctr, seen = base + np.arange(n), np.zeros(n, np.int64), np.zeros((4, 4), np.int64)
    for t in range(steps):
        before, d = cur.cpu().numpy(), done[t].astype(bool)
        books.update(cur, torch.from_numpy(reward[t]).cuda(), torch.from_numpy(done[t]).cuda(), redraw=True, out=cur)
        after = cur.cpu().numpy()
        left, right = pair_draw(seed, gid, ctr, W4)
        assert np.array_equal(after[~d], before[~d]) and np.array_equal(after[d], np.stack([left, right], 1)[d]), t
        assert np.array_equal(after, _expect_out(seed, gid, ctr, W4, before, done[t], True)[0]), t
        np.add.at(seen, (after[d, 0], after[d, 1]), 1)
        ctr += d
    assert np.array_equal(books.env_state()[2].cpu().numpy().view(np.uint32), ctr)
    w = np.asarray(W4)
    print("redraws per cell", seen.tolist(), "table", W4)
    assert ((seen == 0) == (w == 0)).all() and seen[1, 3] > seen[0, 1] > seen[0, 2]  # 5 : 3 : 1 over some thousand draws
    # a table that sums to 0 (floor 0 on a book whose scheduled cells are level): the pair stays, the counter stays
    books.reset()
    books.balance_weights(floor=0)
    assert not books.weights().any()
    before = cur.clone()
    out = books.update(cur, torch.from_numpy(reward[0]).cuda(), torch.ones((n,), dtype=torch.uint8, device="cuda"), redraw=True)
    assert torch.equal(out, before) and torch.equal(books.draw(cur), before)
    assert np.array_equal(books.env_state()[2].cpu().numpy().view(np.uint32), ctr) and books.counters()["episodes"].sum() == n
    with pytest.raises(N.CrlError, match="sum"):
        books.set_weights(np.zeros((4, 4), np.int64))
    with pytest.raises(N.CrlError, match="sum"):
        books.set_weights([[0, 0xFFFFFFFF, 0, 0], [1, 0, 0, 0], [0] * 4, [0] * 4])
    with pytest.raises(ValueError):
        books.set_weights([1, 2, 3, 4])
    with pytest.raises(N.CrlError, match="floor"):
        books.balance_weights(floor=1 << 28)
    books.close()


def test_a_refused_load_leaves_the_books_as_they_were():
    """Counters of the wrong size and an all-zero weight table are refused before anything is written."""
    _need_gpu()
    n, agents, steps = 65, 3, 12
    g = torch.Generator(device="cuda").manual_seed(2)
    books = ArenaBooks(n, agents, "cuda:0", seed=9, env_id_base=40)
    pairs = torch.randint(0, agents, (n, 2), generator=g, device="cuda", dtype=torch.int32)
    for t in range(steps):
        reward = torch.randint(-1, 2, (n,), generator=g, device="cuda").float()
        done = (torch.randint(0, 4, (n,), generator=g, device="cuda") == 0).to(torch.uint8)
        books.update(pairs, reward, done, redraw=True, out=pairs)
    before = books.state_dict()
    assert before["counters"][0].sum() > 0 and before["draw_ctr"].any() and before["ret"].any()
    other = {"agents": agents, "seed": 1234, "counters": before["counters"] + 5, "ignored": before["ignored"] + 1, "ret": before["ret"] + 1,
             "len": before["len"] + 1, "draw_ctr": before["draw_ctr"] + np.uint32(1), "weights": np.arange(9, dtype=np.uint32).reshape(3, 3)}
    for bad in (dict(other, counters=np.zeros((N.CRL_ARENA_COUNTERS, 16, 15), np.int64)), dict(other, weights=np.zeros((3, 3), np.uint32))):
        with pytest.raises(ValueError, match="load_state_dict"):
            books.load_state_dict(bad)
        after = books.state_dict()
        assert sorted(after) == sorted(before)
        for k in before:
            assert np.array_equal(after[k], before[k]), k
    books.close()


def _random_books(rs):
    c = rs.randint(-10 ** 9, 10 ** 9, (N.CRL_ARENA_COUNTERS, 16, 16)).astype(np.int64)
    e = rs.randint(0, 10 ** rs.randint(1, 13, (16, 16)), dtype=np.int64)
    e[0, :3] = [0, 1, 10 ** 6]
    c[0] = e
    return c


def test_balance_weights_on_the_device_equal_the_numpy_rule_bit_for_bit():
    _need_gpu()
    rs = np.random.RandomState(3)
    for agents in (16, 5, 2, 1):
        books = ArenaBooks(70, agents, "cuda:0")
        for trial in range(4):
            own, passed = _random_books(rs), _random_books(rs)
            if trial == 3:  # close books: differences below the cap, and ties
                own[0] = rs.randint(0, 3, (16, 16)) * 30000 + 10 ** 6
            sd = books.state_dict()
            sd["counters"] = own
            books.load_state_dict(sd)
            assert np.array_equal(books.counters_device().cpu().numpy(), own)
            t = torch.from_numpy(passed).cuda()
            for mirror, floor in ((False, 1), (True, 1), (False, 0), (True, 1000)):
                books.balance_weights(mirror, floor)
                assert np.array_equal(books.weights_device().cpu().numpy(), balance_weights_reference(own, agents, mirror, floor).astype(np.int64)), (agents, mirror, floor)
                books.balance_weights(mirror, floor, counters=t)
                assert np.array_equal(books.weights_device().cpu().numpy(), balance_weights_reference(passed, agents, mirror, floor).astype(np.int64)), (agents, mirror, floor)
        if agents == 5:  # the pool grows: entering cells get weight 1 off the diagonal, the table in force stays; then the rule covers them
            books.set_weights(np.arange(25).reshape(5, 5))
            books.set_agents(7)
            grown = np.zeros((16, 16), np.int64)
            grown[:7, :7] = 1 - np.eye(7, dtype=np.int64)
            grown[:5, :5] = np.arange(25).reshape(5, 5)
            assert np.array_equal(books.weights_device().cpu().numpy(), grown)
            books.balance_weights(False, 2)
            assert np.array_equal(books.weights_device().cpu().numpy(), balance_weights_reference(own, 7, False, 2).astype(np.int64))
            books.set_agents(3)
            assert np.array_equal(books.weights_device().cpu().numpy()[:3, :3], balance_weights_reference(own, 7, False, 2)[:3, :3])
            assert books.weights_device().sum() == books.weights_device()[:3, :3].sum()
            # the draw walks the row sums the resize kernel rebuilt
            p = books.draw(torch.zeros((70, 2), dtype=torch.int32, device="cuda")).cpu().numpy()
            left, right = arena_draw_reference(0, np.arange(70), 0, books.weights())
            assert np.array_equal(p, np.stack([left, right], 1))
        books.close()


def _pattern16(n):
    c = np.arange(n) % 16
    return c // 4, c % 4


def test_both_seats_are_served_by_the_right_agent():
    """130 envs (not a multiple of the kernels' groups of 8) on a fixed pair pattern over all 16 cells of [RANDOM, RULE_BASED, WEAK, MEDIUM]:
    for each CNN agent, two crl_policy objects of that agent -- one fed the arena's view-0 frames every step, one view 1 -- must show the
    actions of last_actions[:, seat] on the envs whose seat holds the agent, and the logits to 1e-4; RULE_BASED rows hold 999; RANDOM rows
    are league_draw_reference(seed, 2 * gid + seat, step, CRL_LEAGUE_DOMAIN_ACTION, 3)."""
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps, seed, base = 130, 200, 11, 64
    arena = LeagueArena(_env(n, 4, base), n, POOL4, seed=seed)
    assert arena.env_id_base == base and arena.redraw_on_done
    arena.redraw_on_done = False
    arena.record_logits = True
    left, right = _pattern16(n)
    arena.set_pairs(left, right)
    held = np.stack([left, right], 1)
    pols = {(name, seat): crl.get_compute_action_function(name, n, arena.device) for name in ("WEAK", "MEDIUM") for seat in (0, 1)}
    arena.reset()
    gid = base + np.arange(n)
    worst, checked, ends = 0.0, 0, 0
    for t in range(steps):
        prev = arena._buf
        for (name, seat), pol in pols.items():
            pol.act_device(prev[:, seat], want_logits=True)
        _, _, done = arena.step_device()
        ends += int(done.sum())
        act, logits = arena.last_actions.cpu().numpy(), arena.logits().cpu().numpy().reshape(n, 2, 3)
        for (name, seat), pol in pols.items():
            rows = held[:, seat] == POOL4.index(name)
            assert np.array_equal(act[rows, seat], pol._actions.cpu().numpy()[rows]), (t, name, seat)
            worst = max(worst, float(np.abs(logits[rows, seat] - pol.logits().cpu().numpy()[rows]).max()))
            checked += int(rows.sum())
        for seat in (0, 1):
            assert (act[held[:, seat] == 1, seat] == 999).all(), t
            rows = held[:, seat] == 0
            assert np.array_equal(act[rows, seat], league_draw_reference(seed, 2 * gid[rows] + seat, t, N.CRL_LEAGUE_DOMAIN_ACTION, 3)), (t, seat)
        assert np.array_equal(arena.pairs.cpu().numpy(), held)
    print("both seats: CNN rows checked", checked, "largest logit difference", worst, "episode ends", ends)
    assert worst <= 1e-4 and checked == steps * sum(int((held[:, seat] == a).sum()) for seat in (0, 1) for a in (2, 3)) > 0
    assert arena.counters()["episodes"].sum() == ends  # booked although nothing is redrawn
    arena.close()


# Steps of the real-play run.  Measured on the MI355X with the test's own envs and seeds: the first episode ends at step 104, an episode
# of RULE_BASED against RANDOM lasts 207 wrapped steps on average (125 for RANDOM against itself, 331 for RULE_BASED against itself), and
# 1 200 steps of 257 envs see 1 325 episode ends in 0.3 s
REAL_STEPS = 1200


def test_real_play_through_episode_ends():
    """257 envs of RULE_BASED and RANDOM with mirror matches and redraws: the books equal the numpy replay of the recorded steps, every
    pair change follows the rule, and the seat-symmetrised score is antisymmetric where it is defined."""
    _need_gpu()
    n, seed = 257, 5
    arena = LeagueArena(_env(n, 2), n, ["RULE_BASED", "RANDOM"], seed=seed, include_mirror=True)
    arena.set_weights([[1, 3], [2, 1]])
    arena.reset()
    rec = []
    for t in range(REAL_STEPS):
        before = arena.pairs
        _, rew, done = arena.step_device()
        rec.append((before, rew[:, 0].clone(), done.clone(), arena.pairs))
    replay, gid, ctr, ends, first = Replay(n, 2), np.arange(n), np.zeros(n, np.int64), 0, None
    for t, (before, r, d, after) in enumerate(rec):
        before, r, d, after = before.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool), after.cpu().numpy()
        replay.step(before.astype(np.int64), r, d)
        expect, ctr = _expect_out(seed, gid, ctr, [[1, 3], [2, 1]], before, d, True)
        assert np.array_equal(after, expect), t
        ends += int(d.sum())
        first = t if first is None and d.any() else first
    replay.same_as(arena.books)
    p = arena.payoff()
    print("real play:", REAL_STEPS, "steps, first episode end at step", first, "episode ends", ends, "episodes", p["episodes"].tolist(),
          "score", p["score"].round(3).tolist(), "mean length", p["mean_length"].round(1).tolist())
    assert ends >= 36, "the run must see a few dozen episode ends"
    played = ~np.isnan(p["score"])
    assert played.any() and ((p["score"] + p["score"].T)[played] == 1).all()
    assert not played[0, 1] or p["score"][0, 1] > 0.9  # RULE_BASED beats RANDOM from either seat
    arena.close()


def test_shards_draw_and_book_what_the_whole_batch_does():
    _need_gpu()
    n, agents, steps, seed = 192, 4, 40, 9
    pairs, reward, done = _made_up(n, agents, steps, 6, lo=0, hi=agents)
    whole = ArenaBooks(n, agents, "cuda:0", seed=seed)
    parts = [ArenaBooks(64, agents, "cuda:0", seed=seed, env_id_base=64 * k) for k in range(3)]
    for x in [whole] + parts:
        x.set_weights(W4)
    cur = torch.from_numpy(pairs[0]).cuda()
    cuts = [cur[64 * k:64 * (k + 1)].clone() for k in range(3)]
    for t in range(steps):
        r, d = torch.from_numpy(reward[t]).cuda(), torch.from_numpy(done[t]).cuda()
        whole.update(cur, r, d, redraw=True, out=cur)
        for k, x in enumerate(parts):
            x.update(cuts[k], r[64 * k:64 * (k + 1)], d[64 * k:64 * (k + 1)].contiguous(), redraw=True, out=cuts[k])
        assert torch.equal(cur, torch.cat(cuts)), t
    c, cs = whole.counters(), [x.counters() for x in parts]
    assert c["episodes"].sum() > 500 and not torch.equal(cur.cpu(), torch.from_numpy(pairs[0]))
    for k in NAMES:
        assert np.array_equal(c[k], sum(x[k] for x in cs)), k
    for j in range(3):
        assert torch.equal(torch.cat([x.env_state()[j] for x in parts]), whole.env_state()[j])
    for x in [whole] + parts:
        x.close()


def test_a_fresh_arena_continues_from_a_state_dict():
    """The books alone on made-up steps, then a whole LeagueArena (RULE_BASED, WEAK, MEDIUM) with its env: the copy shows the actions,
    rewards, flags, pairs and books of the original."""
    _need_gpu()
    n, agents, steps = 777, 4, 30
    pairs, reward, done = _made_up(n, agents, 2 * steps, 8, lo=0, hi=agents)
    dev = [(torch.from_numpy(reward[t]).cuda(), torch.from_numpy(done[t]).cuda()) for t in range(2 * steps)]
    a = ArenaBooks(n, agents, "cuda:0", seed=6, env_id_base=1000)
    a.set_weights(W4)
    cur = torch.from_numpy(pairs[0]).cuda()
    for t in range(steps):
        a.update(cur, *dev[t], redraw=True, out=cur)
    a.balance_weights(False, 1)
    b = ArenaBooks(n, agents, "cuda:0", seed=999, env_id_base=1000)
    b.load_state_dict(a.state_dict())
    other = cur.clone()
    for t in range(steps, 2 * steps):
        a.update(cur, *dev[t], redraw=True, out=cur), b.update(other, *dev[t], redraw=True, out=other)
        assert torch.equal(cur, other), t
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb) and sa["draw_ctr"].any() and sa["counters"][0].sum() > steps
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.close(), b.close()

    n, names = 131, ["RULE_BASED", "WEAK", "MEDIUM"]
    a = LeagueArena(_env(n, 3), n, names, seed=4)
    a.reset()
    _near_the_end(a.env)
    for t in range(steps):
        a.step_device()
    b = LeagueArena(_env(n, 3), n, names, seed=1234)
    b.reset()
    b.env.load_state_dict(a.env.state_dict())
    before = b.pairs
    for bad in (dict(a.state_dict(), obs=np.zeros((1, 2, 1, 42, 42), np.uint8)), dict(a.state_dict(), pairs=np.full((n, 2), 3)),
                dict(a.state_dict(), stack=np.zeros((n, 4, 42, 42), np.uint8))):
        with pytest.raises(ValueError, match="load_state_dict"):
            b.load_state_dict(bad)
        assert torch.equal(b.pairs, before) and b.books.state_dict()["seed"] == 1234 and not b.counters()["episodes"].any()  # as it was
    b.load_state_dict(a.state_dict())
    ends = 0
    for t in range(steps):
        (ba, ra, da), (bb, rb, db) = a.step_device(), b.step_device()
        assert torch.equal(a.last_actions, b.last_actions) and torch.equal(ba, bb) and torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(a.pairs, b.pairs), t
        ends += int(da.sum())
    ca, cb = a.counters(), b.counters()
    assert ends > 0 and all(np.array_equal(ca[k], cb[k]) for k in NAMES) and ca["episodes"].sum() >= ends
    a.close(), b.close()


def test_step_device_does_no_host_work():
    """The method of tests/test_hip_ledger.py::test_step_device_with_a_ledger_does_no_host_work: 50 arena steps with books, redraws and a
    balance_weights() call every 10 steps, enqueued behind a long-running launch, leave the host before that launch ends."""
    _need_gpu()
    n = 4096
    arena = LeagueArena(_env(n, 3), n, POOL4, seed=1)
    arena.reset()
    _near_the_end(arena.env)
    arena.draw_pairs()
    for t in range(10):  # warm-up: lazy allocations, kernel loading
        arena.step_device()
    arena.balance_weights()
    x = torch.randn((8192, 8192), device=arena.device)
    y = torch.empty_like(x)
    torch.mm(x, x, out=y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.mm(x, x, out=y)
    torch.cuda.synchronize()
    reps = int(max(8, min(400, 1.5 / (time.perf_counter() - t0))))  # about 1.5 s of queued work
    for _ in range(reps):
        torch.mm(x, x, out=y)
    busy = torch.cuda.Event()
    busy.record()
    t0 = time.perf_counter()
    for t in range(10, 60):
        prev = arena.step_device()
        if t % 10 == 0:
            arena.balance_weights()
    host = time.perf_counter() - t0
    still_busy = not busy.query()
    torch.cuda.synchronize()
    print("50 arena step_device calls took the host", round(host * 1e3, 2), "ms behind", reps, "queued matrix products; device still busy:", still_busy)
    assert still_busy, "the host waited for the device inside step_device"
    assert prev[0].shape == (n, 2, 1, 42, 42) and arena.counters()["episodes"].sum() > 0
    arena.close()


def test_books_at_65536_envs_on_512_sampled_envs():
    """One run at full size on made-up steps: the whole counter table, `ignored` and all pairs against the numpy replay and the rule, the
    per-env state on 512 sampled envs."""
    _need_gpu()
    n, agents, steps, seed = 65536, 6, 24, 2
    table = np.random.RandomState(5).randint(0, 9, (agents, agents))
    pairs, reward, done = _made_up(n, agents, steps, 4)
    books = ArenaBooks(n, agents, "cuda:0", seed=seed)
    books.set_weights(table)
    rows = np.sort(np.random.RandomState(6).choice(n, 512, replace=False))
    replay, gid, ctr = Replay(n, agents), np.arange(n), np.zeros(n, np.int64)
    for t in range(steps):
        out = books.update(torch.from_numpy(pairs[t]).cuda(), torch.from_numpy(reward[t]).cuda(), torch.from_numpy(done[t]).cuda(), redraw=True)
        expect, ctr = _expect_out(seed, gid, ctr, table, pairs[t], done[t], True)
        assert np.array_equal(out.cpu().numpy(), expect), t
        replay.step(pairs[t].astype(np.int64), reward[t, :, 0], done[t])
    replay.same_as(books, rows)
    c = books.counters()
    print("65 536 envs: episodes", int(c["episodes"].sum()), "ignored", c["ignored"])
    assert c["episodes"].sum() + c["ignored"] == int(done.sum()) and c["ignored"] > 0 and (c["episodes"] > 0).all()
    assert np.array_equal(books.env_state()[2].cpu().numpy().view(np.uint32)[rows], ctr[rows])
    books.close()


def test_play_fills_every_scheduled_cell_and_a_tiny_budget_returns_cleanly():
    _need_gpu()
    n = 64
    arena = LeagueArena(_env(n, 7), n, ["RULE_BASED", "RANDOM"], seed=3)
    assert arena.pairs.cpu().numpy().tolist() == [[0, 1], [1, 0]] * 32  # env g starts on the (g mod cells)-th scheduled pair
    p = arena.play(episodes_per_pair=1, max_steps=3)
    assert np.isnan(p["win_rate"]).all() and np.isnan(p["score"]).all() and not p["episodes"].any()
    p = arena.play(episodes_per_pair=1, max_steps=REAL_STEPS, check_every=64)
    off = ~np.eye(2, dtype=bool)
    print("play: episodes", p["episodes"].tolist(), "win rate", p["win_rate"].tolist(), "mean length", p["mean_length"].tolist())
    assert (p["episodes"][off] >= 1).all() and not np.diag(p["episodes"]).any() and np.isnan(np.diag(p["win_rate"])).all()
    assert p["win_rate"][0, 1] > 0.9 and p["win_rate"][1, 0] < 0.1 and p["score"][0, 1] + p["score"][1, 0] == 1
    arena.redraw_on_done = False
    with pytest.raises(ValueError, match="redraw_on_done"):
        arena.play(episodes_per_pair=1, max_steps=10)
    arena.redraw_on_done = True
    obs, rew, done, info = arena.step()  # the host protocol books as well
    assert len(obs) == 2 and tuple(rew.shape) == (n, 2) and arena.counters()["length_sum"].sum() >= p["episodes"].sum()
    with pytest.raises(ValueError, match="not in the pool"):
        arena.set_pairs("WEAK", 0)
    with pytest.raises(ValueError, match="index agent_names"):
        arena.set_pairs(np.full(n, 2), 0)
    from competitive_rl_amd.policy_serving import BUILTIN_CHECKPOINTS

    arena.set_weights([[0, 1], [1, 0]])
    arena.add_agent("MINE", BUILTIN_CHECKPOINTS["WEAK"])
    assert arena.weights().tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]] and arena.counters()["episodes"].shape == (3, 3)
    with pytest.raises(ValueError, match="full-size"):
        arena.add_agent("BIG", {"conv3_w": np.zeros(1)})
    arena.close()

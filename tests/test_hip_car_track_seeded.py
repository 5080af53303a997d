"""cCarRacing: the tracks of a SEEDED context against the written rule (include/crl.h "car track draws", restated in
``rules.car_track_draws``) walked by the CPU oracle -- bit for bit, as every track comparison here (both sides walk with
include/crl_f64.h).  The other tests of the seeded path compare the device with itself (pipelined against CRL_CAR_NO_OVERLAP, shards
against the batch, walk-ahead piece sizes against each other); the tests that use the oracle replay draws handed to both sides.  Here
the draws come from the rule alone: Philox counter and key (high words of the env id and of the seed included), the 53-bit uniforms,
the swap bit of the attempt that closed the lap (the birth places in the compared state prove it), the episode index of full resets,
inline auto-resets, stored and unfinished walk-aheads, and what ``seed()`` / ``set_replay()`` leave behind.

Cases and expected tracks: tests/car_track_cases.py; what they hold and which fault each catches: tests/test_car_track_rules.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STORED = 130  # steps after which the next episode's walk is stored (test_set_state_that_rewinds...: one piece of 160 iterations per step)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@pytest.fixture(scope="module")
def text():
    _need_gpu()
    from competitive_rl_amd import _native as N
    from oracle import car_oracle as co

    co.set_text(N.load_car_text())
    yield
    co.set_text(None)


def make_env(n, seed, base=0, inline=False, **kw):
    import competitive_rl_amd as crl

    if not inline:
        return crl.HipCarVecEnv(n, seed=seed, env_id_base=base, **kw)
    os.environ["CRL_CAR_NO_OVERLAP"] = "1"  # read at create: this context walks every track inside its reset kernel
    try:
        return crl.HipCarVecEnv(n, seed=seed, env_id_base=base, **kw)
    finally:
        del os.environ["CRL_CAR_NO_OVERLAP"]


def check_tracks(env, E, where, idx=None, obs=None, deep=3, players=2):
    """envs ``idx`` of the HIP env against the oracle records E (one per listed env): track length, tiles, border flags with their
    white / red parity, start pose; for the first ``deep`` the map (nothing outside the window) and, given ``obs``, the first frames"""
    from tests import car_track_cases as K

    idx = np.arange(env.num_envs) if idx is None else np.asarray(idx)
    assert len(idx) == len(E)
    for j, i in enumerate(idx):
        tr, e = env.get_track(int(i)), E[j]
        nt = int(e["trk"]["n"])
        assert tr["n"] == nt, (where, "track length", int(i), tr["n"], nt)
        bad = (tr["tile_poly"] != e["tile32"][:nt]).reshape(nt, -1).any(1)
        assert not bad.any(), (where, "tile_poly", int(i), "tiles", np.nonzero(bad)[0][:8])
        border = np.where(e["trk"]["border"][:nt] > 0, np.where(np.arange(nt) % 2 == 0, 1, 2), 0).astype(np.uint8)
        assert np.array_equal(tr["border"], border), (where, "border flags", int(i), np.nonzero(tr["border"] != border)[0][:8])
        pose = e["trk"]["track"][0][1:4].astype(np.float32)
        assert np.array_equal(tr["start_pose"], pose), (where, "start pose", int(i), tr["start_pose"], pose)
    for j, i in enumerate(idx[:deep]):
        o = K.oracle_env(E[j])
        m, overflow = env.get_map(int(i))
        assert overflow == 0 and np.array_equal(m, o.map()), (where, "map", int(i), overflow, int((m != o.map()).sum()))
        if obs is not None:
            for v in range(players):
                want = o.render(v)
                assert np.array_equal(obs[i, v], want), (where, "first frame", int(i), v, int((obs[i, v] != want).sum()))


def check(env, E, where, idx=None, obs=None, next_episode=None, deep=3):
    """check_tracks and the whole car state (bodies, joints, wheel model, tile books, manifolds): the birth places prove the swap bit"""
    from tests.test_hip_car_episodes import assert_state_equal

    idx = np.arange(env.num_envs) if idx is None else np.asarray(idx)
    check_tracks(env, E, where, idx, obs, deep)
    hs = env.get_state()[idx]
    assert_state_equal(hs, E, where)
    assert (hs["elapsed"] == 0).all(), (where, "elapsed")
    if next_episode is not None:
        assert np.array_equal(hs["episode"].astype(np.int64), np.asarray(next_episode, np.int64)), (where, "episode", hs["episode"][:8])


def end_episodes(env, which=None, episodes=None):
    """TimeLimit's last step for the envs ``which`` (all by default), optionally with the episode indices (the NEXT track's) set
    through set_state first; returns the observations, the first frames of the new episodes among them"""
    n = env.num_envs
    which = np.ones(n, bool) if which is None else which
    st = env.get_state()
    st["elapsed"][which] = 999
    if episodes is not None:
        st["episode"] = episodes
    env.set_state(st)
    obs, _, done = env.step_device(torch.zeros((n, 2, 2), device="cuda"))
    assert np.array_equal(done.cpu().numpy().astype(bool), which), "exactly the picked envs end"
    return obs.cpu().numpy()


def run(env, steps):
    """steps with the cars standing; the host waits for each, so that every step queues its piece of the walk-ahead"""
    act = torch.zeros((env.num_envs, 2, 2), device="cuda")
    for _ in range(steps):
        _, _, done = env.step_device(act)
        assert not bool(done.any().item())


@pytest.mark.parametrize("case", range(6))
def test_full_reset_follows_the_written_rule(text, case):
    """reset() of a seeded context: episode 0 of (seed, env_id_base + i) -- with the env id and the seed above 2^32, and at 1, 65 and
    130 envs (the reset kernel takes a wavefront per env, the walk a lane per env)"""
    from tests import car_track_cases as K

    assert len(K.RESET_CASES) == 6
    name, seed, base, n = K.RESET_CASES[case]
    env = make_env(n, seed, base)
    obs = env.reset().cpu().numpy()
    E, att, swap = K.expected_batch(seed, [base + i for i in range(n)], np.zeros(n, np.int64))
    check(env, E, ("reset()", name), obs=obs, next_episode=np.ones(n))
    if n >= 65:
        assert (att > 1).sum() >= 3 and 0 < swap.sum() < n, (name, att, swap)
    env.close()


def test_inline_auto_resets_follow_the_written_rule(text):
    """A context without walk-ahead (CRL_CAR_NO_OVERLAP=1: every walk inside the reset kernel, lane 0 of the env's wavefront).  The
    episode indices are set through set_state -- 2^20 - 1 and 2^20 among them: the counter keeps the episode's low 20 bits, so (gid 1,
    episode 2^20) is (gid 1, episode 0), two attempts -- and every env's TimeLimit ends; the new episodes are compared."""
    from tests import car_track_cases as K

    n = K.INLINE_N
    env = make_env(n, K.SEED, inline=True)
    obs = env.reset().cpu().numpy()
    E, _, _ = K.expected_batch(K.SEED, range(n), np.zeros(n, np.int64))
    check(env, E, "reset(), no walk-ahead", obs=obs, next_episode=np.ones(n), deep=1)
    eps = K.inline_episodes(n)
    obs = end_episodes(env, episodes=eps.astype(np.uint32))
    E, att, _ = K.expected_batch(K.SEED, range(n), eps)
    assert att[1] == 2 and att[2] == 2 and att[80] == 3
    check(env, E, "inline auto-reset", obs=obs, next_episode=eps + 1, deep=4)
    env.close()


@pytest.mark.parametrize("n", [65, 130])
def test_auto_resets_from_the_walk_ahead_follow_the_written_rule(text, n):
    """The default, pipelined context: the walk of an env's NEXT episode is laid beside the steps in pieces of 160 iterations, kept
    in a WalkSave between pieces and taken by the reset when its tag equals the episode.  Which path a reset took cannot be observed
    from outside (a reset whose walk is not there walks inline, and results never depend on it -- that is the point), so the run is
    shaped for the stored walk: STORED = 130 steps between resets, the host waiting for every step, is what
    test_set_state_that_rewinds... takes for the walks to be in -- 130 pieces x 160 = 20 800 iterations against at most 3 attempts x
    2 500 for the slowest env of these batches (gid 80, episode 1; tests/test_car_track_rules.py), were even a third of the pieces
    skipped.  Three consecutive auto-resets of every env are compared, the envs whose first and second attempts fail included, and
    the envs of ``early`` are ended once more two steps after a reset: the inline fallback beside an unfinished walk."""
    from tests import car_track_cases as K

    env = make_env(n, K.SEED)
    obs = env.reset().cpu().numpy()
    ep = np.zeros(n, np.int64)  # the episode each env is in

    def compare(where, idx=None, deep=2):
        idx = np.arange(n) if idx is None else idx
        E, att, _ = K.expected_batch(K.SEED, idx, ep[idx])
        check(env, E, (where, n), idx=idx, obs=obs, next_episode=ep[idx] + 1, deep=deep)
        return att

    compare("reset()")
    early = K.early(n)
    tried = 0
    for rnd in (1, 2, 3):
        run(env, STORED)
        obs = end_episodes(env)
        ep += 1
        tried += int((compare(("walk-ahead", rnd)) > 1).sum())
        if rnd == 1:
            run(env, 2)
            obs = end_episodes(env, which=early)
            ep[early] += 1
            compare("two steps after a reset", idx=np.nonzero(early)[0])
    assert tried >= 5 and ep.max() == 4
    assert env.cap_hits() == (0, 0, 0, 0)
    env.close()


def test_rekeying_voids_stored_and_unfinished_walks(text):
    """seed() and set_replay() change what the draws are a function of while walks of the old key are stored or half done
    (invalidate_walks): with episode 1 walked ahead under seed A, seed(B) makes the next tracks those of (B, gid, 1); with episode 2
    under way under B, set_replay() makes it the replayed draws' at index (16 * 2 + attempt) mod attempts; with episode 3 stored from
    the replay stream, set_replay(None) puts the env back on the Philox rule under B."""
    from oracle import car_oracle as co
    from tests import car_track_cases as K

    n, A = 65, 48
    env = make_env(n, K.SEED)
    env.reset()
    run(env, STORED)  # episode 1 is stored under K.SEED
    env.seed(K.SEED_B)
    obs = end_episodes(env)
    E, _, _ = K.expected_batch(K.SEED_B, range(n), np.ones(n, np.int64))
    check(env, E, "after seed(B)", obs=obs, next_episode=np.full(n, 2))
    stale, _, _ = K.expected_batch(K.SEED, range(n), np.ones(n, np.int64))
    assert all(K.signature(E[i]) != K.signature(stale[i]) for i in range(n))  # (what a walk kept from before seed() would have given)

    run(env, 5)  # episode 2 under B is under way
    rs = np.random.RandomState(41)
    u, swap = rs.random_sample((n, A, 24)), rs.randint(0, 2, (n, A)).astype(np.uint8)
    env.set_replay(u, swap)
    obs = end_episodes(env)
    E = np.zeros(n, co.ENV_DT)
    for i in range(n):
        o, draws = co.CarEnv(), u[i, 32:48].reshape(-1)  # (16 * episode 2 + attempt) mod 48
        att = o.reset(draws, 0)
        assert att > 0, ("no attempt of the replayed draws closes a lap", i)
        o.reset(draws, int(swap[i, 32 + att - 1]))
        o.e["contacts_enabled"] = 1
        o.step(None)
        E[i] = o.buf[0]
    check(env, E, "after set_replay(u, swap)", obs=obs, next_episode=np.full(n, 3))

    run(env, STORED)  # episode 3 of the replay stream is stored
    env.set_replay(None, None)
    obs = end_episodes(env)
    E, _, _ = K.expected_batch(K.SEED_B, range(n), np.full(n, 3, np.int64))
    check(env, E, "after set_replay(None)", obs=obs, next_episode=np.full(n, 4))
    env.close()


def test_one_player_context_gets_the_same_tracks_and_birth_place_0(text):
    """cCarRacing-v0 under the same key: the double env's tracks, the car at birth place 0 whatever the swap bit says -- the state of
    the oracle's car that drew place 0 (the cars do not touch: each one's reset + step(None) is its own)"""
    from tests import car_track_cases as K
    from tests.test_hip_car_episodes import BODY

    for seed, base, n in ((K.SEED, (1 << 32) + 5, 3), (K.SEED, 5, 3)):
        one, two = make_env(n, seed, base, players=1), make_env(n, seed, base)
        one.reset(), two.reset()
        E, _, swap = K.expected_batch(seed, [base + i for i in range(n)], np.zeros(n, np.int64))
        assert swap.any()
        check_tracks(one, E, ("one player", base), deep=1)
        s1 = one.get_state()
        for i in range(n):
            t1, t2 = one.get_track(i), two.get_track(i)
            assert t1["n"] == t2["n"] and np.array_equal(t1["tile_poly"], t2["tile_poly"]) and np.array_equal(t1["border"], t2["border"])
            q, o = s1[i]["car"][0], E[i]["car"][int(swap[i])]  # swap = 1: car 1 of the double env starts from place 0
            for f in BODY:
                assert q["hull"][f] == o["hull"][f] and np.array_equal(q["wheel"][f], o["wheel"][f]), ("one player", base, i, f)
        one.close(), two.close()

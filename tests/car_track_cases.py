"""Seeded CarRacing tracks as the WRITTEN rule gives them: the cases shared by tests/test_car_track_rules.py (CPU) and
tests/test_hip_car_track_seeded.py (GPU).  Everything here comes from ``rules.car_track_draws`` (include/crl.h "car track
draws") and the CPU oracle; nothing reads the device.

A reset of (seed, gid, episode) draws attempts 0, 1, ... until one closes a lap (car_oracle_reset over the draws of 16
attempts), takes THAT attempt's swap bit for the birth places and ends with CarRacing.reset's step(None).  The oracle costs
milliseconds per reset and the tests share hundreds of them: results are cached per key and computed on first use."""
import functools
import hashlib

import numpy as np

from competitive_rl_amd import rules as R
from oracle import car_oracle as co

ATTEMPTS = 16  # draws handed to the oracle per reset; no case needs more than three
SEED = 11
SEED_HI = (7 << 32) | 11  # a key whose high word is not zero (its low word is SEED)
SEED_B = (3 << 32) | 5  # the key the re-keying test moves to
WRAP = 1 << 20  # episode e and e + 2^20 share their counters

# (name, seed, env_id_base, n, episodes): contexts whose full reset() / auto-resets are compared with the oracle
CASES = (
    ("gid above 2^32", SEED, (1 << 32) + 5, 3, (0,)),
    ("gid above 2^40", SEED, (1 << 40) + 1, 1, (0,)),
    ("seed above 2^32", SEED_HI, 0, 3, (0,)),
    ("one env", SEED, 0, 1, (0,)),
    ("65 envs", SEED, 0, 65, (0, 1, 2, 3)),
    ("130 envs", SEED, 0, 130, (0, 1, 2, 3)),
)
RESET_CASES = tuple((name, seed, base, n) for name, seed, base, n, _ in CASES)  # reset(): episode 0 of each
WALK_AHEAD_SIZES = (65, 130)  # auto-resets from the walk-ahead: episodes 1, 2, 3 of seed SEED
HISTOGRAM_KEYS = tuple((SEED, g, e) for e in range(3) for g in range(130))  # the 390 resets of docs/LAB_NOTES_car_track_draws.md


def early(n):
    """envs the walk-ahead test ends a second time two steps after their reset (they run one episode ahead of the others)"""
    return np.arange(n) % 5 == 3


INLINE_N = 130


def inline_episodes(n=INLINE_N):
    """the episodes the inline auto-reset test sets through set_state: the NEXT track's index per env"""
    ep = 1 + (np.arange(n) % 2)
    ep[1], ep[2], ep[3] = WRAP, WRAP - 1, 0
    return ep.astype(np.int64)


def compared_keys():
    """every (seed, gid, episode) the GPU tests compare with the oracle, the small special contexts first"""
    keys = []
    for _, seed, base, n, _ in CASES[:3]:
        keys += [(seed, base + i, 0) for i in range(n)]
    keys += [(SEED, i, int(e)) for i, e in enumerate(inline_episodes())]
    for n in (1,) + WALK_AHEAD_SIZES:
        keys += [(SEED, i, 0) for i in range(n)]
    for n in WALK_AHEAD_SIZES:
        for rnd in (1, 2, 3):
            keys += [(SEED, i, rnd) for i in range(n)]
        keys += [(SEED, int(i), 4) for i in np.nonzero(early(n))[0]]
    keys += [(SEED_B, i, e) for e in (1, 3) for i in range(65)]
    return list(dict.fromkeys(keys))


def reset_under(draws, seed, gid, episode, swap_from="closing"):
    """Oracle env after the reset ``draws(seed, gid, episode, attempts) -> (u [A, 24], swap [A])`` describes: (attempts used,
    swap used, swap of attempt 0, env record) -- attempts -1 and no record when none of the 16 closes a lap."""
    u, swap = draws(seed, gid, episode, range(ATTEMPTS))
    o = co.CarEnv()
    att = o.reset(u.reshape(-1), 0)
    if att <= 0:
        return -1, -1, int(swap[0]), None
    sw = int(swap[att - 1] if swap_from == "closing" else swap[0])
    if sw:
        assert o.reset(u.reshape(-1), sw) == att
    o.e["contacts_enabled"] = 1
    o.step(None)
    rec = o.buf.copy()
    rec.flags.writeable = False  # (cached and shared: nobody steps it)
    return att, sw, int(swap[0]), rec[0]


@functools.lru_cache(maxsize=None)
def expected(seed, gid, episode):
    """(attempts, swap, swap of attempt 0, oracle env record after reset + step(None)) of the written rule"""
    att, sw, sw0, e = reset_under(R.car_track_attempts, int(seed), int(gid), int(episode))
    assert att > 0, ("no attempt closes a lap", seed, gid, episode)
    return att, sw, sw0, e


def expected_batch(seed, gids, episodes):
    """oracle env array (car_oracle.ENV_DT) of the listed envs, attempts and swap bits"""
    got = [expected(seed, int(g), int(e)) for g, e in zip(gids, episodes)]
    E = np.zeros(len(got), co.ENV_DT)
    for i, g in enumerate(got):
        E[i] = g[3]
    return E, np.array([g[0] for g in got]), np.array([g[1] for g in got])


def oracle_env(record):
    """a CarEnv over a copy of a cached record (map, render)"""
    o = co.CarEnv()
    o.buf[0] = record
    return o


def signature(record):
    """what a fault in the draws can change: the track's tiles and the two birth places"""
    if record is None:
        return None
    n = int(record["trk"]["n"])
    h = hashlib.sha256(record["tile32"][:n].tobytes())
    for c in range(2):
        for f in ("cx", "cy", "a"):
            h.update(record["car"][c]["hull"][f].tobytes())
    return n, h.hexdigest()


def tile_digest(record):
    n = int(record["trk"]["n"])
    return hashlib.sha256(record["tile32"][:n].tobytes()).hexdigest()[:16]

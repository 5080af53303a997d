"""The built-in CarRacing drivers on the CPU (include/crl.h "car drivers"): known answers of the numpy restatement
``rules.car_driver_reference`` (what the GPU tests compare ``car_driver_kernel`` with, bit for bit), the RANDOM draws, the rule's
quality closed loop through the CPU checker, and the argument refusals of the ``crl_car_driver_*`` entry points."""
import ctypes

import numpy as np
import pytest

from competitive_rl_amd import car_driver_reference, get_builtin_car_driver_names
from competitive_rl_amd import rules as R

F = np.float32
DEFAULT = dict(R.CAR_DRIVER_DEFAULT_STYLE)


def car_at(cx, cy, hx=0.0, hy=1.0, vx=0.0, vy=0.0):
    """hull [1, 4] and wheels [1, 4, 2] of a car at (cx, cy) whose heading is the unit vector (hx, hy): wheels at the reference's
    WHEELPOS (+-55, +80 / -82) * SIZE, rotated"""
    lx, ly = hy, -hx  # the car's right-hand side
    pos = [(-1.1, 1.6), (1.1, 1.6), (-1.1, -1.64), (1.1, -1.64)]
    wheels = np.array([[[cx + a * lx + b * hx, cy + a * ly + b * hy] for a, b in pos]], F)
    return np.array([[cx, cy, vx, vy]], F), wheels


def row_of_tiles(k, step=3.5, half=6.5):
    """k boxes in a row along +y, tile t centred on (0, step * t + step / 2)"""
    b = np.zeros((1, k, 4), F)
    b[0, :, 0], b[0, :, 2] = -half, half
    b[0, :, 1], b[0, :, 3] = step * np.arange(k), step * np.arange(k) + step
    return b


def act(hull, wheels, boxes, n=None, done=0, style=None, seed=0, gid=0, car=0, call=0):
    n = boxes.shape[1] if n is None else n
    return car_driver_reference(hull, wheels, done, boxes, n, DEFAULT if style is None else style, seed, gid, car, call)


def test_names_and_default_style():
    assert get_builtin_car_driver_names() == ("RANDOM", "RULE_BASED")
    assert R.check_car_style() == DEFAULT and DEFAULT["epsilon"] == 0.0
    for bad in (dict(kind="FAST"), dict(target_speed=-1.0), dict(target_speed=float("nan")), dict(steer_gain=float("inf")), dict(lookahead=65),
                dict(lookahead=-1), dict(lookahead=2.5), dict(epsilon=1.5), dict(epsilon=-0.1)):
        with pytest.raises(ValueError):
            R.check_car_style(**bad)


def test_straight_row_gives_zero_steer_and_gas():
    hull, wheels = car_at(0.0, 1.75)
    a = act(hull, wheels, row_of_tiles(12))
    assert a.dtype == F and a.shape == (1, 2)
    assert a[0, 0] == 0.0 and a[0, 1] > 0


def test_mirrored_inputs_mirror_the_steer_bit_for_bit():
    rs = np.random.RandomState(5)
    E, T = 64, 40
    boxes = np.zeros((E, T, 4), F)
    lo = rs.uniform(-100, 100, (E, T, 2)).astype(F)
    boxes[..., :2], boxes[..., 2:] = lo, lo + rs.uniform(1, 8, (E, T, 2)).astype(F)
    hull = rs.uniform(-100, 100, (E, 4)).astype(F)
    wheels = (hull[:, None, :2] + rs.uniform(-2, 2, (E, 4, 2))).astype(F)
    n = rs.randint(1, T + 1, E)
    soft = dict(DEFAULT, steer_gain=0.5)  # inside the clamp: the steer carries the sine's bits
    a = car_driver_reference(hull, wheels, 0, boxes, n, soft, 0, np.arange(E), 0, 0)
    mb = boxes[..., [2, 1, 0, 3]] * np.array([-1, 1, -1, 1], F)  # x -> -x: the box's x bounds swap
    mh, mw = hull * np.array([-1, 1, -1, 1], F), wheels * np.array([-1, 1], F)
    m = car_driver_reference(mh, mw, 0, mb, n, soft, 0, np.arange(E), 0, 0)
    assert np.array_equal(m[:, 0].view(np.uint32), (-a[:, 0]).view(np.uint32)) and np.array_equal(m[:, 1].view(np.uint32), a[:, 1].view(np.uint32))
    assert (np.abs(a[:, 0]) > 0).sum() > E // 2 and len(np.unique(a[:, 0])) > E // 4  # (not all at the target-behind values or zero)


def test_distance_tie_takes_the_lower_index():
    hull, wheels = car_at(0.0, 0.0)
    left, right = [-7.0, -1.0, -3.0, 1.0], [3.0, -1.0, 7.0, 1.0]  # centres (-5, 0) and (5, 0): the same distance from the car
    style = dict(DEFAULT, lookahead=0)
    a = act(hull, wheels, np.array([[left, right]], F), style=style)
    b = act(hull, wheels, np.array([[right, left]], F), style=style)
    assert a[0, 0] == -1.0 and b[0, 0] == 1.0  # steer > 0 turns right: the target is tile 0 both times


def test_done_car_and_empty_track_get_zero():
    hull, wheels = car_at(3.0, 1.0, vx=5.0)
    for style in (DEFAULT, dict(kind="RANDOM"), dict(DEFAULT, epsilon=1.0)):
        assert np.array_equal(act(hull, wheels, row_of_tiles(6), done=1, style=style), np.zeros((1, 2), F))
        assert np.array_equal(act(hull, wheels, row_of_tiles(6), n=0, style=style), np.zeros((1, 2), F))


def test_clamps_engage():
    hull, wheels = car_at(0.0, 0.0, vy=100.0)
    a = act(hull, wheels, np.array([[[3.0, -1.0, 7.0, 1.0]]], F), style=dict(DEFAULT, lookahead=0, steer_gain=40.0))
    assert a[0, 0] == 1.0 and a[0, 1] == -1.0  # steer_gain * 1 and (45 * 0.5 - 100) * 0.1 both lie far outside
    hull, wheels = car_at(0.0, 0.0)
    a = act(hull, wheels, np.array([[[-7.0, -1.0, -3.0, 1.0]]], F), style=dict(DEFAULT, lookahead=0, steer_gain=40.0))
    assert a[0, 0] == -1.0 and a[0, 1] == 1.0
    a = act(hull, wheels, row_of_tiles(9), style=dict(DEFAULT, steer_gain=0.5, target_speed=4.0))
    assert a[0, 0] == 0.0 and a[0, 1] == F(F(4.0) * F(0.1))  # inside the clamp the value itself comes out


def test_lookahead_wraps_modulo_n():
    k = 7
    ang = 2 * np.pi * np.arange(k) / k
    c = np.stack([30 * np.cos(ang), 30 * np.sin(ang)], axis=1)
    boxes = np.concatenate([c - 2, c + 2], axis=1).astype(F)[None]
    hull, wheels = car_at(28.0, -3.0, hx=0.6, hy=0.8)  # nearest: tile 0
    soft = dict(DEFAULT, steer_gain=0.25)
    for la in (0, 1, 3, 6):
        want = act(hull, wheels, boxes[:, [(0 + la) % k]], style=dict(soft, lookahead=0))  # a track of the target tile alone
        for wrapped in (la, la + k, la + 2 * k):
            got = act(hull, wheels, boxes, style=dict(soft, lookahead=wrapped))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (la, wrapped)
    outs = {act(hull, wheels, boxes, style=dict(soft, lookahead=la)).tobytes() for la in range(k)}
    assert len(outs) > 3  # (the targets differ)


def test_philox_mapping_known_answers():
    # Random123's known-answer test of philox4x32_10: counter 0, key 0
    x = R._philox4x32_10(0, 0, 0, 0)
    assert [int(w) for w in x] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    u = R.car_driver_unit(np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0x80000100, 0xFFFFFFFF], np.uint64))
    assert u.dtype == F
    assert u.tolist() == [-1.0, -1.0, -1.0 + 2.0 ** -23, -(2.0 ** -23), 0.0, 2.0 ** -23, 1.0 - 2.0 ** -23]
    # the counter layout: (gid lo, gid hi, call, domain + car) under (seed lo, seed hi)
    gid, seed, call = (5 << 32) | 7, (9 << 32) | 11, 13
    for car in (0, 1):
        w = R.car_driver_draws(seed, gid, car, call)
        c = [np.uint64(7), np.uint64(5), np.uint64(13), np.uint64(0x43524430 + car)]
        k0, k1 = 11, 9
        for _ in range(10):
            p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
            m = np.uint64(0xFFFFFFFF)
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        assert [int(a) for a in w] == [int(a) for a in c]
    hull, wheels = car_at(0.0, 0.0)
    a = act(hull, wheels, row_of_tiles(3), style=dict(kind="RANDOM"), seed=seed, gid=gid, car=1, call=call)
    w = R.car_driver_draws(seed, gid, 1, call)
    assert a[0].tolist() == [float(R.car_driver_unit(w[0])), float(R.car_driver_unit(w[1]))] and (-1 <= a).all() and (a < 1).all()


def test_random_does_not_depend_on_the_batch_split():
    rs = np.random.RandomState(2)
    E = 130
    hull = rs.uniform(-50, 50, (E, 4)).astype(F)
    wheels = (hull[:, None, :2] + rs.uniform(-2, 2, (E, 4, 2))).astype(F)
    boxes = np.repeat(row_of_tiles(20), E, axis=0)
    for style in (dict(kind="RANDOM"), dict(DEFAULT, epsilon=0.5)):
        for car in (0, 1):
            whole = car_driver_reference(hull, wheels, 0, boxes, 20, style, 77, np.arange(E), car, 4)
            halves = [car_driver_reference(hull[s], wheels[s], 0, boxes[s], 20, style, 77, base + np.arange(65), car, 4)
                      for s, base in ((slice(0, 65), 0), (slice(65, 130), 65))]
            assert np.array_equal(whole, np.concatenate(halves))
        assert len(np.unique(whole[:, 0])) > 60
    a0 = car_driver_reference(hull, wheels, 0, boxes, 20, dict(kind="RANDOM"), 77, np.arange(E), 0, 4)
    for other in (dict(seed=78), dict(car=1), dict(call=5)):
        kw = dict(dict(seed=77, car=0, call=4), **other)
        assert not np.array_equal(a0, car_driver_reference(hull, wheels, 0, boxes, 20, dict(kind="RANDOM"), kw["seed"], np.arange(E), kw["car"], kw["call"]))


def test_epsilon_threshold_at_zero_and_one():
    rs = np.random.RandomState(3)
    E = 200
    hull = rs.uniform(-20, 20, (E, 4)).astype(F)
    wheels = (hull[:, None, :2] + rs.uniform(-2, 2, (E, 4, 2))).astype(F)
    boxes = np.repeat(row_of_tiles(20), E, axis=0)
    args = (hull, wheels, 0, boxes, 20)
    ruled = car_driver_reference(*args, dict(DEFAULT, epsilon=0.0), 1, np.arange(E), 0, 9)
    rnd = car_driver_reference(*args, dict(kind="RANDOM"), 1, np.arange(E), 0, 9)
    assert np.array_equal(car_driver_reference(*args, dict(DEFAULT, epsilon=1.0), 1, np.arange(E), 0, 9), rnd)  # eps_q = 0xFFFFFFFF
    assert not np.array_equal(ruled, rnd)
    assert R.sample_eps_q(0.0) == 0 and R.sample_eps_q(1.0) == 0xFFFFFFFF
    x2 = R.car_driver_draws(1, np.arange(E), 0, 9)[2]
    for eps in (0.25, 0.5):
        mixed = car_driver_reference(*args, dict(DEFAULT, epsilon=eps), 1, np.arange(E), 0, 9)
        explore = x2 < np.uint64(R.sample_eps_q(eps))
        assert np.array_equal(mixed, np.where(explore[:, None], rnd, ruled)) and 0 < explore.sum() < E


# ---- the rule's quality, closed loop through the CPU checker
TRACKS, STEPS = 8, 1000
# REGRESSION PIN of the numpy rule (not a property of the env): tiles visited per track and car after 1000 steps with both cars on the
# default RULE_BASED style, as recorded in docs/LAB_NOTES_car_drivers.md; a change of the rule or of its constants moves them
PINNED_VISITED = [[234, 243], [244, 231], [227, 240], [245, 235], [231, 242], [244, 234], [234, 245], [240, 226]]


def _bodies(E, c):
    car = E["car"][:, c]
    hull = np.stack([car["hull"][k] for k in ("cx", "cy", "vx", "vy")], axis=1)
    return hull, np.stack([car["wheel"]["cx"], car["wheel"]["cy"]], axis=2)


def closed_loop(styles, steps=STEPS, tracks=TRACKS, seed=3):
    """Both cars of `tracks` seeded tracks through oracle.car_oracle.CarBatch; styles[c]: a style dict, or a constant action.
    Returns (tiles visited [tracks, 2], tile counts, left-the-playfield flags [tracks, 2], done flags)."""
    from oracle import car_oracle as co
    from tests.car_scenarios import make_oracle_envs

    envs = make_oracle_envs(tracks, seed0=0)
    B = co.CarBatch(tracks)
    for i in range(tracks):
        B.E[i] = envs[i].e
    n = B.E["trk"]["n"].astype(np.int64)
    boxes = B.E["tile_aabb"].copy()
    for i in range(tracks):  # the checker keeps the float32 boxes the device keeps
        assert np.array_equal(boxes[i, :n[i]], R.car_tile_boxes(B.E["tile32"][i, :n[i]]))
    left = np.zeros((tracks, 2), bool)
    for t in range(steps):
        acts = np.zeros((tracks, 2, 2), F)
        for c in range(2):
            if isinstance(styles[c], dict):
                hull, wheels = _bodies(B.E, c)
                acts[:, c] = car_driver_reference(hull, wheels, B.E["done"][:, c], boxes, n, styles[c], seed, np.arange(tracks), c, t)
            else:
                acts[:, c] = styles[c]
        B.step(acts.astype(np.float64))
        for c in range(2):
            h = B.E["car"][:, c]["hull"]
            left[:, c] |= (np.abs(h["cx"]) > 2000 / 6.0) | (np.abs(h["cy"]) > 2000 / 6.0)  # PLAYFIELD (car_racing_multi_players.py:593)
    return B.E["tile_visited_count"].copy(), n, left, B.E["done"].copy()


def test_rule_based_outdrives_full_gas_and_random_on_every_track():
    ruled, n, left, _ = closed_loop([DEFAULT, DEFAULT])
    base, n2, _, _ = closed_loop([(0.0, 1.0), dict(kind="RANDOM")])  # car 0 under constant (0, +1), car 1 RANDOM, the same tracks
    assert np.array_equal(n, n2)
    share = ruled / n[:, None]
    print("tiles per track", n.tolist())
    print("RULE_BASED visited", ruled.tolist())
    print("constant (0, +1) visited", base[:, 0].tolist(), "RANDOM visited", base[:, 1].tolist())
    print("share of the track reached: min %.3f median %.3f" % (share.min(), np.median(share)))
    assert not left.any(), "a RULE_BASED car left the playfield"
    for c in range(2):
        assert (ruled[:, c] > base[:, 0]).all() and (ruled[:, c] > base[:, 1]).all(), (ruled.tolist(), base.tolist())
    assert ruled.tolist() == PINNED_VISITED  # the regression pin (see above)


def test_abi_refuses_bad_arguments_without_gpu():
    from competitive_rl_amd import _native as N

    L = N.load()
    h = ctypes.c_void_p()
    err = lambda: L.crl_last_error()  # noqa: E731
    assert L.crl_car_driver_create(None, 0, ctypes.byref(h)) == -1 and b"null" in err()
    assert L.crl_car_driver_create(None, 0, None) == -1
    ok = (1, 45.0, 4, 1.5, 0.0)  # kind, target_speed, lookahead, steer_gain, epsilon
    assert L.crl_car_driver_set_style(None, 1, *ok) == -1 and b"null driver" in err()
    for slot in (-1, 16):
        assert L.crl_car_driver_set_style(None, slot, *ok) == -1 and b"slot" in err()
        assert L.crl_car_driver_get_style(None, slot, None, None, None, None, None) == -1 and b"slot" in err()
    for kind in (-1, 2):
        assert L.crl_car_driver_set_style(None, 1, kind, 45.0, 4, 1.5, 0.0) == -1 and b"kind" in err()
    for ts in (-1.0, float("nan"), float("inf")):
        assert L.crl_car_driver_set_style(None, 1, 1, ts, 4, 1.5, 0.0) == -1 and b"target_speed" in err()
        assert L.crl_car_driver_set_style(None, 1, 1, 45.0, 4, ts, 0.0) == -1 and b"steer_gain" in err()
    for la in (-1, 65):
        assert L.crl_car_driver_set_style(None, 1, 1, 45.0, la, 1.5, 0.0) == -1 and b"lookahead" in err()
    for eps in (-0.5, 1.5, float("nan")):
        assert L.crl_car_driver_set_style(None, 1, 1, 45.0, 4, 1.5, eps) == -1 and b"epsilon" in err()
    assert L.crl_car_driver_get_style(None, 1, None, None, None, None, None) == -1
    assert L.crl_car_driver_set_assignment(None, None, None) == -1 and L.crl_car_driver_get_assignment(None, None, None) == -1
    assert L.crl_car_driver_act(None, None, None) == -1 and b"null" in err()
    assert L.crl_car_driver_get_counters(None, None, None) == -1
    assert L.crl_car_driver_set_counters(None, 0, -1) == -1 and b"calls" in err()
    assert L.crl_car_driver_set_counters(None, 0, 1 << 32) == -1 and L.crl_car_driver_set_counters(None, 0, 0) == -1
    L.crl_car_driver_destroy(None)

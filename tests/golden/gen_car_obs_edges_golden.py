"""Golden vectors for the CarRacing observation where the view leaves the map window.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_car_obs_edges_golden.py

Same provenance and layout as the C8 fixture of ``gen_car_obs_golden.py`` (its ``put_state`` is used here): every recorded
frame is the return value of the reference's own ``CarRacing.get_observation`` over the pygame / Box2D stand-ins of
``_car_render_standins.py``, drawn from its full 10000 x 10000 ``observation_playground``.  One track (seed 100 of that
generator); the body states are SYNTHETIC inputs: a car at rest is moved rigidly (hull and four wheels, float32) so that

* ``edge``    the camera centre (hull position + 16 units ahead, in map pixels) lies at a given distance from one side of the
              window [4392, 5608)^2 that the product and the checker keep of the surface: fully inside, partial, fully
              outside, and both sides of the +-160 px distance beyond which the product draws plain grass; at four quarter-turn
              view angles (pygame's rotate90) and two general ones (the 16.16 rotation);
* ``vel``     the same distances with the view angle set by a velocity above 0.5 (atan2(-vx, vy)) instead of the heading;
* ``corner``  the camera at the window's corners;
* ``field``   the hull at |x| or |y| = 333.0 / 333.3 / 333.4 units (the playfield boundary that ends an episode), heading
              outward and along the boundary;
* ``far``     a car 900 / 1500 units away;
* ``ind``     cars at rest on the track with extreme indicator inputs (wheel speeds up to +-4000, speed 100, hull w = +-78.5,
              steering +-0.42) and rewards on the rounding edges of "%05.0f";
* ``sweep``   car 1 placed through viewer 0's screen: across rows 31/32 and 63/64, on each screen edge, over viewer 0's car.

``car_obs_edges.npz``: the 24-draw attempts of the track; per frame the cars' state (oracle ``CAR_DT`` records + rewards), the
two observations (96, 96) uint8, a tag, and per view the group description ``vtag`` = "group|where|angle|offset".
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _car_render_standins as R  # noqa: E402
from _car_standins import Draws  # noqa: E402
from gen_car_obs_golden import put_state  # noqa: E402

from oracle import car_oracle as co  # noqa: E402  (only to hold the input states)

ATLAS = os.path.join(ROOT, "competitive_rl_amd", "assets", "car_reward_text.npz")
f32 = np.float32

SCALE = (10 / (100 / np.sqrt(96.0))) * 1.8  # map pixels per unit (car_racing_multi_players.py:214-215)
WIN_LO, WIN_HI = 4392, 5608
OFFSETS = [-140, -70, -30, 0, 30, 70, 100, 150, 160, 170, 200, 330]  # map px outward from the window side
ANGLES = [0.0, float(f32(np.pi / 2)), float(f32(np.pi)), float(f32(-np.pi / 2)), 0.785, -2.7]
SIDES = ["x_lo", "x_hi", "y_lo", "y_hi"]
REWARDS = [0.5, 1.5, 2.5, -0.5, -1.5, -0.0, 999.5]


def rigid(o, base, c, origin, heading, steer=0.0):
    """car c of `base` moved rigidly, in float32, so that its hull's body origin is `origin` and its heading `heading`; at rest"""
    o.e["car"] = base
    p0 = o.hull_position(c)[:2].astype(f32)
    q = o.e["car"][c]
    a0 = f32(q["hull"]["a"])
    d = f32(f32(heading) - a0)
    cs, sn = f32(np.cos(d)), f32(np.sin(d))
    ox, oy = f32(origin[0]), f32(origin[1])
    bodies = [q["hull"]] + [q["wheel"][w] for w in range(4)]
    for k, b in enumerate(bodies):
        rx, ry = f32(b["cx"] - p0[0]), f32(b["cy"] - p0[1])
        b["cx"], b["cy"] = f32(ox + f32(f32(cs * rx) - f32(sn * ry))), f32(oy + f32(f32(sn * rx) + f32(cs * ry)))
        rel = f32(b["a"] - a0) + (f32(steer) if k in (1, 2) else f32(0))
        b["a"] = f32(heading) if k == 0 else f32(f32(heading) + rel)
        b["vx"] = b["vy"] = b["w"] = 0
    q["omega"][:] = 0
    return q.copy()


def origin_for_camera(px, view_angle):
    """hull origin (units) that puts the camera centre at map pixel `px` when the view angle is `view_angle`"""
    off = ((5000.0 - px[0]) / SCALE, (5000.0 - px[1]) / SCALE)
    return off[0] + np.sin(view_angle) * 16.0, off[1] - np.cos(view_angle) * 16.0


def side_px(side, offset, t):
    """camera pixel `offset` px outward of `side`, at tangential map coordinate t"""
    if side == "x_lo":
        return WIN_LO - offset, t
    if side == "x_hi":
        return WIN_HI + offset, t
    if side == "y_lo":
        return t, WIN_LO - offset
    return t, WIN_HI + offset


def main():
    holder = {"seed": 100}

    def stream(seed):
        d = Draws(holder["seed"])
        holder["draws"] = d
        return d

    cd, cr = R.load_car_reference(stream, ATLAS)
    env = cr.CarRacing(num_player=2, verbose=0)
    d = holder["draws"]
    before = len(d.u)
    env.reset()
    u = np.array(d.u[before:])
    assert len(u) % 24 == 0
    o = co.CarEnv(libm=True)
    assert o.reset(u, 0) == len(u) // 24
    nt = int(o.e["trk"]["n"])
    assert nt == len(env.track) and np.array_equal(np.array(env.track), o.e["trk"]["track"][:nt]), "oracle track != reference track"
    o.e["contacts_enabled"] = 1
    o.step(None)
    base = o.e["car"].copy()
    for c in range(2):  # at rest
        q = base[c]
        for b in [q["hull"]] + [q["wheel"][w] for w in range(4)]:
            b["vx"] = b["vy"] = b["w"] = 0
        q["omega"][:] = 0
    trk = np.array(env.track)[:, 2:4]  # (x, y) of the track's points, units
    # tangential map coordinate per side: where the track comes closest to that side
    tang = {"x_lo": 5000.0 - SCALE * trk[np.argmax(trk[:, 0]), 1], "x_hi": 5000.0 - SCALE * trk[np.argmin(trk[:, 0]), 1],
            "y_lo": 5000.0 - SCALE * trk[np.argmax(trk[:, 1]), 0], "y_hi": 5000.0 - SCALE * trk[np.argmin(trk[:, 1]), 0]}
    frames = []

    def record(tag, cars, rewards, vtags):
        o.e["car"] = np.stack(cars)
        o.e["reward"][:] = rewards
        put_state(env, o)
        obs = np.stack([env.get_observation(i)[..., 0] for i in range(2)])
        frames.append((o.e["car"].copy(), o.e["reward"].copy(), obs, tag, list(vtags)))

    def at_camera(c, px, ang):
        return rigid(o, base, c, origin_for_camera(px, ang), ang)

    # ---- window sides: car 0 on one side, car 1 on the opposite one
    for s0, s1 in (("x_lo", "x_hi"), ("y_lo", "y_hi")):
        for ai, ang in enumerate(ANGLES):
            for off in OFFSETS:
                cars = [at_camera(0, side_px(s0, off, tang[s0]), ang), at_camera(1, side_px(s1, off, tang[s1]), ang)]
                record(f"edge/{s0}+{s1}/a{ai}/{off:+d}", cars, [0.0, 0.0], [f"edge|{s0}|a{ai}|{off:+d}", f"edge|{s1}|a{ai}|{off:+d}"])
    # ---- the view angle from the velocity (speed 30), not from the heading (0.3 / -1.1)
    for off in OFFSETS:
        cars = []
        for c, (side, va, head) in enumerate((("x_lo", 2.2, 0.3), ("y_hi", -0.6, -1.1))):
            # camera = hull position + R(view angle) (0, 16): the hull origin for that, with this heading
            q = rigid(o, base, c, origin_for_camera(side_px(side, off, tang[side]), va), head)
            q["hull"]["vx"], q["hull"]["vy"] = f32(-30.0 * np.sin(va)), f32(30.0 * np.cos(va))
            cars.append(q)
        record(f"vel/x_lo+y_hi/{off:+d}", cars, [0.0, 0.0], [f"vel|x_lo|v|{off:+d}", f"vel|y_hi|v|{off:+d}"])
    # ---- window corners: 0 and +70 px outward on both axes, three angles
    corners = {"lo_lo": ("x_lo", "y_lo"), "hi_hi": ("x_hi", "y_hi"), "lo_hi": ("x_lo", "y_hi"), "hi_lo": ("x_hi", "y_lo")}

    def corner_px(name, off):
        sx, sy = corners[name]
        return side_px(sx, off, 0)[0], side_px(sy, off, 0)[1]

    for c0, c1 in (("lo_lo", "hi_hi"), ("lo_hi", "hi_lo")):
        for ai in (0, 4, 5):
            for off in (0, 70):
                cars = [at_camera(0, corner_px(c0, off), ANGLES[ai]), at_camera(1, corner_px(c1, off), ANGLES[ai])]
                record(f"corner/{c0}+{c1}/a{ai}/{off:+d}", cars, [0.0, 0.0], [f"corner|{c0}|a{ai}|{off:+d}", f"corner|{c1}|a{ai}|{off:+d}"])
    # ---- the playfield boundary: hull position at |x| or |y| = 333.0 / 333.3 / 333.4, heading outward / along
    along = {"+x": float(trk[np.argmax(trk[:, 0]), 1]), "-x": float(trk[np.argmin(trk[:, 0]), 1]),
             "+y": float(trk[np.argmax(trk[:, 1]), 0]), "-y": float(trk[np.argmin(trk[:, 1]), 0])}
    outward = {"+x": -np.pi / 2, "-x": np.pi / 2, "+y": 0.0, "-y": np.pi}  # heading h points along (-sin h, cos h)

    def field_origin(where, dist):
        t = along[where]
        return {"+x": (dist, t), "-x": (-dist, t), "+y": (t, dist), "-y": (t, -dist)}[where]

    for w0, w1 in (("+x", "-x"), ("+y", "-y")):
        for dist in (333.0, 333.3, 333.4):
            # outward; along the boundary.  "Along" is 1.3 rad from outward and not pi / 2: the outward headings are quarter turns and
            # take pygame's rotate90, a second quarter turn would take it again; at 1.3 the view runs along the boundary (the window's
            # edge crosses the screen lengthwise) through the 16.16 rotation
            for hi, turn in enumerate((0.0, 1.3)):
                cars = [rigid(o, base, 0, field_origin(w0, dist), outward[w0] + turn), rigid(o, base, 1, field_origin(w1, dist), outward[w1] + turn)]
                h = "out" if hi == 0 else "along"
                record(f"field/{w0}{w1}/{dist}/{h}", cars, [0.0, 0.0], [f"field|{w0}|{h}|{dist}", f"field|{w1}|{h}|{dist}"])
    # ---- far cars: +900 units (what the wrapper tests do to a car) and -1500
    def shifted(c, dx, dy):
        q = base[c].copy()
        for b in [q["hull"]] + [q["wheel"][w] for w in range(4)]:
            b["cx"], b["cy"] = f32(b["cx"] + f32(dx)), f32(b["cy"] + f32(dy))
        return q

    record("far/car1+900x", [base[0].copy(), shifted(1, 900.0, 0.0)], [12.0, -100.0], ["far|track|-|0", "far|+900x|-|0"])
    record("far/car0-1500x/car1+900y", [shifted(0, -1500.0, 0.0), shifted(1, 0.0, 900.0)], [-3.0, 7.0], ["far|-1500x|-|0", "far|+900y|-|0"])
    # ---- indicator extremes and read-out rounding: cars at rest on the track
    def ind(c, omega=None, speed=None, w=None, steer=0.0):
        o.e["car"] = base
        q = rigid(o, base, c, o.hull_position(c)[:2], base[c]["hull"]["a"], steer=steer)
        if omega is not None:
            q["omega"][:] = omega
        if speed is not None:
            q["hull"]["vx"], q["hull"]["vy"] = f32(0.6 * speed), f32(0.8 * speed)
        if w is not None:
            q["hull"]["w"] = f32(w)
        return q

    ind_frames = [
        ("omega320", ind(0, omega=[320, -320, 320, -320]), ind(1, omega=[-320, 320, -320, 320])),
        ("speed100+w78.5", ind(0, speed=100.0), ind(1, w=78.5)),
        ("w-78.5+steer0.42", ind(0, w=-78.5), ind(1, steer=0.42)),
        ("steer-0.42+omega1300", ind(0, steer=-0.42), ind(1, omega=[1300, -1300, 1300, -1300])),
        ("omega-1300+omega2000", ind(0, omega=[-1300, 1300, -1300, 1300]), ind(1, omega=[2000, -2000, 2000, -2000])),
        ("omega-2000+omega4000", ind(0, omega=[-2000, 2000, -2000, 2000]), ind(1, omega=[4000, -4000, 4000, -4000])),
        ("omega-4000+mixed", ind(0, omega=[-4000, 4000, -4000, 4000]), ind(1, omega=[1300, 2000, 4000, 320])),
    ]
    for k, (name, q0, q1) in enumerate(ind_frames):
        record(f"ind/{name}", [q0, q1], [REWARDS[k], REWARDS[(k + 3) % 7]], [f"ind|{name}|0|0", f"ind|{name}|1|0"])
    # ---- car 1 swept through viewer 0's screen: its hull origin at the world point that the camera transform maps to (X, Y)
    o.e["car"] = base
    a0 = float(base[0]["hull"]["a"])
    hp = o.hull_position(0)[:2].astype(np.float64)
    cam = hp + np.array([-np.sin(a0) * 16.0, np.cos(a0) * 16.0])

    def world_of(X, Y):  # inverse of Car.draw_for_pygame's  -scale * R(-angle) (w - off) + 48
        tx, ty = (48.0 - X) / SCALE, (48.0 - Y) / SCALE
        return cam[0] + np.cos(a0) * tx - np.sin(a0) * ty, cam[1] + np.sin(a0) * tx + np.cos(a0) * ty

    targets = [(X, Y) for Y in (32, 64) for X in (8, 30, 70, 90)]
    targets += [(X, Y) for X in (0, 95) for Y in (10, 32, 50, 64, 80)]
    targets += [(X, 0) for X in (0, 20, 48, 95)] + [(X, 95) for X in (0, 40, 95)]
    targets += [(48, 76), (45, 74), (51, 79), (48, 70), (44, 80), (52, 72), (48, 83)]  # over viewer 0's own car (drawn at about (48, 76))
    targets += [(31, 31), (64, 64), (2, 93), (93, 2), (47, 32), (49, 63), (1, 33), (94, 62)]
    turns = [0.0, 0.7, float(f32(np.pi / 2)), -2.3]
    for k, (X, Y) in enumerate(targets):
        cars = [base[0].copy(), rigid(o, base, 1, world_of(X, Y), a0 + turns[k % 4])]
        record(f"sweep/{X}/{Y}/t{k % 4}", cars, [0.0, 0.0], [f"sweep|{X},{Y}|t{k % 4}|0", f"sweep1|{X},{Y}|t{k % 4}|0"])

    out = {"draws": u}
    out["cars"] = np.stack([f[0] for f in frames])
    out["reward"] = np.stack([f[1] for f in frames])
    out["obs"] = np.stack([f[2] for f in frames])
    out["tag"] = np.array([f[3] for f in frames])
    out["vtag"] = np.array([f[4] for f in frames])
    path = os.path.join(HERE, "car_obs_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "frames", len(frames), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()

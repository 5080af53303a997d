"""cCarRacingDouble frames where the view leaves the map window, in every draw form of the product, against the frames recorded
from the reference (tests/golden/car_obs_edges.npz) and against the CPU oracle -- tolerance 0, no frame left out.

What the fixture holds and why it would notice a wrong kernel: tests/test_oracle_car_obs_edges_golden.py.  The draw forms:
  (a) the big launch (car_obs_third_kernel, a third of a tile per wavefront): set_state + render_current;
  (b) the whole-tile list form (car_obs_list_kernel): terminal frames and the first frames of new episodes;
  (c) the long-list thirds form (car_view_list_kernel + car_obs_third_list_kernel): envs whose cars touch or are near each other;
  (d) done_policy="car0": a finished car 1 that stays in the world outside the playfield, drawn on every step;
  (e) players=1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_hip_car_episodes import _park_beside, batch_to_hip_state  # noqa: E402
from tests.test_hip_car_parity import oracle_to_hip_state, push_tracks  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BODIES = ("hull", "wheel")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


class Edges:
    """the fixture, the oracle env of its track, and the oracle's own frames (drawn once per module)"""

    def __init__(self):
        from competitive_rl_amd import _native as N
        from oracle import car_oracle as co

        self.co = co
        co.set_text(N.load_car_text())
        g = np.load(os.path.join(G, "car_obs_edges.npz"))
        self.g, self.draws = g, g["draws"]
        self.tags = [str(t) for t in g["tag"]]
        self.group = [t.split("/")[0] for t in self.tags]
        self.F = len(self.tags)
        e = co.CarEnv()
        assert e.reset(self.draws, 0) == len(self.draws) // 24
        e.e["contacts_enabled"] = 1
        e.step(None)
        self.base = e
        self.map = e.map()
        self.oracle_obs = np.zeros((self.F, 2, 96, 96), np.uint8)
        self.stays = []  # frames whose car 0 is inside the playfield (its episode goes on) while its view leaves the window
        for i in range(self.F):
            e.e["car"], e.e["reward"] = g["cars"][i], g["reward"][i]
            for v in range(2):
                self.oracle_obs[i, v] = e.render(v)
            if self.group[i] in ("edge", "vel", "corner", "field") and self.leaves_window(e, 0) and np.abs(e.hull_position(0)[:2]).max() < 333.2:
                self.stays.append(i)
        e.e["car"], e.e["reward"] = g["cars"][self.tags.index("far/car1+900x")], 0.0  # (car 0 of that frame is the car at rest on the track)
        self.on_track = e.e["car"].copy()
        # the frames that the stepping tests use: every fifth, all far / indicator frames, and the cars over each other left out of
        # the steps (two hulls placed inside each other are no state the step can reach)
        pick = set(range(0, self.F, 5)) | {i for i in range(self.F) if self.group[i] in ("far", "ind")}
        over_own_car = {i for i in range(self.F) if self.group[i] == "sweep" and self.tags[i].split("/")[1:3] in
                        (["48", "76"], ["45", "74"], ["51", "79"], ["48", "70"], ["44", "80"], ["52", "72"], ["48", "83"])}
        self.subset = sorted(pick - over_own_car)
        assert 48 <= len(self.subset) <= 62 and {self.group[i] for i in self.subset} == set(self.group), len(self.subset)

    def leaves_window(self, env, v):
        """does viewer v of the oracle env sample a pixel outside the map window"""
        src, _ = env.view_sources(v)
        return bool(((src < self.co.MAP_ORG) | (src >= self.co.MAP_ORG + self.co.MAP_W)).any())

    def twin(self, cars, reward):
        tw = self.co.CarEnv()
        tw.buf[:] = self.base.buf
        tw.e = tw.buf[0]
        tw.e["car"], tw.e["reward"] = cars, reward
        return tw

    def twins(self, frames):
        return [self.twin(self.g["cars"][i], self.g["reward"][i]) for i in frames]

    def batch(self, twins):
        B = self.co.CarBatch(len(twins))
        for i, tw in enumerate(twins):
            B.E[i] = tw.e
        return B

    def render(self, B, i, v):
        return B.view(i).render(v, self.map)  # (every env is on the one track: one map)

    def oracle_reset(self, B, i):
        o = B.view(i)
        assert o.reset(self.draws, 0) == len(self.draws) // 24
        o.e["contacts_enabled"] = 1
        o.step(None)


@pytest.fixture(scope="module")
def edges():
    _need_gpu()
    ed = Edges()
    yield ed
    ed.co.set_text(None)


def make_hip(ed, twins, **kw):
    """a HIP env per oracle twin, all on the fixture's track; every later episode replays the same draws (the same track)"""
    import competitive_rl_amd as crl

    n = len(twins)
    hip = crl.HipCarVecEnv(n, seed=1, **kw)
    A = len(ed.draws) // 24
    hip.set_replay(np.broadcast_to(ed.draws.reshape(1, A, 24), (n, A, 24)), np.zeros((n, A), np.uint8))
    hip.reset()
    push_tracks(hip, twins)
    return hip


def mismatches(got, want, names):
    """[(name, viewer, differing pixels)] over (n, V, 96, 96) frames"""
    bad = []
    for i in range(len(want)):
        for v in range(want.shape[1]):
            d = int((got[i, v] != want[i, v]).sum())
            if d:
                bad.append((names[i], v, d))
    return bad


def fixtures_paired(co, e):
    """The product's "could the cars touch" test on an oracle env's poses (car_step.hip fixtures_near): the world boxes of the eight
    fixtures of each car (four hull polygons, four wheels), each grown by 0.04, overlap for some pair that is not wheel and wheel.
    (float64 here, hardware sine / cosine there: the spacings of these tests are 0.02 or more away from the rule's edge.)"""
    K = co.consts()
    boxes = []
    for c in range(2):
        car, bb = e["car"][c], []
        for f in range(8):
            b = car["hull"] if f < 4 else car["wheel"][f - 4]
            lc = K["hull_lc"].astype(np.float64) if f < 4 else np.zeros(2)
            v = (K["hull_poly"][f][:K["hull_n"][f]] if f < 4 else K["wheel_poly"]).astype(np.float64)
            sn, cs = np.sin(float(b["a"])), np.cos(float(b["a"]))
            R = np.array([[cs, -sn], [sn, cs]])
            w = v @ R.T + (np.array([float(b["cx"]), float(b["cy"])]) - R @ lc)
            bb.append((w[:, 0].min() - 0.04, w[:, 1].min() - 0.04, w[:, 0].max() + 0.04, w[:, 1].max() + 0.04))
        boxes.append(bb)
    return any(not (a[0] > b[2] or b[0] > a[2] or a[1] > b[3] or b[1] > a[3])
               for fa, a in enumerate(boxes[0]) for fb, b in enumerate(boxes[1]) if fa < 4 or fb < 4)


def step_and_compare(ed, hip, B, names, elapsed, steps, actions, car0=False):
    """`steps` steps of HIP env and oracle batch side by side: rewards, done flags, every terminal observation, every returned frame
    (for an env that finished: the first frame of its new episode), and the manifold count of every env that goes on.  Returns per env
    the steps at which it finished, and per step: the oracle's manifold counts, which views left the map window (both before the
    finished envs were reset), and whether the poses the step started from pair the cars (fixtures_paired)."""
    n = B.n
    finished, manifolds, partial, paired = [[] for _ in range(n)], [], [], []
    acts = np.ascontiguousarray(actions, np.float32)
    for t in range(steps):
        paired.append(np.array([fixtures_paired(ed.co, B.E[i]) for i in range(n)]))
        obs, rew, done = hip.step_device(torch.as_tensor(acts).cuda())
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
        r, d = B.step(acts.astype(np.float64))
        elapsed += 1
        want_done = (d[:, 0] > 0 if car0 else d.any(1)) | (elapsed >= 1000)
        assert np.array_equal(rew, r.astype(np.float32)), ("reward", t, [names[i] for i in np.nonzero((rew != r.astype(np.float32)).any(1))[0]][:8])
        assert np.array_equal(done, want_done), ("done", t, [names[i] for i in np.nonzero(done != want_done)[0]][:8])
        manifolds.append(B.E["n_contact"].copy())
        partial.append(np.array([[ed.leaves_window(B.view(i), v) for v in range(2)] for i in range(n)]))
        fin = np.nonzero(want_done)[0]
        if len(fin):
            term = torch.stack(hip.terminal_observation(torch.as_tensor(fin).cuda())).cpu().numpy()
            want = np.stack([[ed.render(B, i, v) for v in range(2)] for i in fin])
            bad = mismatches(term, want, [names[i] for i in fin])
            assert not bad, ("terminal_observation", t, bad[:10])
            for i in fin:
                ed.oracle_reset(B, i)
                elapsed[i] = 0
                finished[i].append(t)
        want = np.stack([[ed.render(B, i, v) for v in range(2)] for i in range(n)])
        bad = mismatches(obs, want, [names[i] + ("/new episode" if want_done[i] else "") for i in range(n)])
        assert not bad, ("frame after step", t, bad[:10])
        got, on = hip.get_state()["n_contact"], ~want_done
        assert np.array_equal(got[on], B.E["n_contact"][on]), ("n_contact", t, [names[i] for i in np.nonzero(on & (got != B.E["n_contact"]))[0]][:8])
    return finished, manifolds, partial, paired


def test_big_launch_equals_recording_and_oracle(edges):
    """(a) one env per recorded frame, set_state, render_current: car_obs_third_kernel with the checked background, the far tile,
    bars that cross the thirds' boundaries, car spans on the first and last row of a third."""
    ed = edges
    twins = ed.twins(range(ed.F))
    hip = make_hip(ed, twins)
    hip.set_state(oracle_to_hip_state(twins))
    got = hip.render_current().cpu().numpy()
    bad = mismatches(got, ed.g["obs"], ed.tags)
    assert not bad, ("against the recording", len(bad), bad[:12])
    bad = mismatches(got, ed.oracle_obs, ed.tags)
    assert not bad, ("against the oracle", len(bad), bad[:12])
    hip.close()


def test_whole_tile_list_form_terminal_and_first_frames(edges):
    """(b) every env at elapsed 999: one step ends all episodes, the terminal frames and the new episodes' first frames come from
    car_obs_list_kernel.  Two more envs end the way production episodes end: a car crosses |x| = 333.3 during a step and is found
    outside at the next one -- once with the cars alone, once wheel to wheel.  The wheel-to-wheel env has a manifold at the first
    step; the contact pushes the cars 0.02 apart, so at the step that ends the episode the cars are paired (fixtures_paired: the
    product solves them as one island, the env finishes "while coupled") without a manifold."""
    ed = edges
    frames = ed.subset
    names = [ed.tags[i] for i in frames] + ["crossing/alone", "crossing/wheel to wheel"]
    out = ed.tags.index("field/+x-x/333.0/out")  # car 0 at x = +333.0 heading +x, car 1 at x = -333.0 heading -x
    twins = ed.twins(frames) + ed.twins([out, out])
    B = ed.batch(twins)
    n = B.n
    for i in (n - 2, n - 1):
        for c, vx in ((0, 30.0), (1, -30.0)):  # 0.6 units per step outward
            for b in BODIES:
                B.E["car"][i, c][b]["vx"] = vx
    _park_beside(B.E, np.array([n - 1]))
    for i in (n - 2, n - 1):
        assert abs(float(B.view(i).hull_position(0)[0])) < 2000 / 6 < abs(float(B.view(i).hull_position(0)[0])) + 0.6
    elapsed = np.full(n, 999, np.int64)
    elapsed[n - 2:] = 10
    hip = make_hip(ed, twins)
    hip.set_state(batch_to_hip_state(B.E, elapsed, np.zeros(n, np.int64)))
    finished, manifolds, _, paired = step_and_compare(ed, hip, B, names, elapsed, 2, np.zeros((n, 2, 2), np.float32))
    assert all(f and f[0] == 0 for f in finished[:n - 2]), "every pose ends its episode at the first step"
    assert finished[n - 2] == [1] and finished[n - 1] == [1], ("the crossing cars are found outside at the second step", finished[n - 2:])
    assert manifolds[0][n - 1] > 0 and paired[0][n - 1] and paired[1][n - 1], "the wheel-to-wheel env is coupled at both steps, the one that ends it included"
    assert manifolds[0][n - 2] == 0 and not paired[0][n - 2] and not paired[1][n - 2], "the other env's cars are alone"
    assert hip.cap_hits() == (0, 0, 0, 0)
    hip.close()


@pytest.mark.parametrize("gap,touching", [(2.6, True), (2.67, False)])
def test_long_list_thirds_form(edges, gap, touching):
    """(c) car 1 parked beside car 0 of every pose -- car_view_list_kernel + car_obs_third_list_kernel draw these envs' frames.
    gap 2.6: wheel to wheel, a manifold at the first step (the touching envs); the contact pushes the cars apart, so the later steps
    find them near each other without a manifold.  gap 2.67: the parked cars are 0.055 apart (the oracle finds manifolds up to gap
    2.63, separation 0.02): beyond Box2D's contact margin of 0.02, inside the 0.08 by which the product's pairing test grows the
    boxes (car_step.hip fixtures_near) -- paired, no manifold: the near-only envs from the first step on.  A car that moves (spinning
    hull, spinning wheels, a velocity) may run into its neighbour later; the cars at rest must not.
    The poses: the stepping subset, and every recorded pose whose car 0 is still inside the playfield while its view leaves the window
    -- the only partial views this form can be asked for, since a car outside the playfield ends the episode."""
    ed = edges
    frames = ed.subset + [i for i in ed.stays if i not in ed.subset][:64 - len(ed.subset)]
    twins = ed.twins(frames)
    B = ed.batch(twins)
    n = B.n
    hull = B.E["car"][:, 0]["hull"]
    at_rest = (hull["vx"] == 0) & (hull["vy"] == 0) & (hull["w"] == 0) & (B.E["car"][:, 0]["omega"] == 0).all(1)
    _park_beside(B.E, np.arange(n), gap=gap)
    elapsed = np.full(n, 10, np.int64)
    hip = make_hip(ed, twins)
    hip.set_state(batch_to_hip_state(B.E, elapsed, np.zeros(n, np.int64)))
    names = [ed.tags[i] for i in frames]
    finished, manifolds, partial, paired = step_and_compare(ed, hip, B, names, elapsed, 3, np.zeros((n, 2, 2), np.float32))
    assert np.array_equal(hip.get_state()["n_contact"], B.E["n_contact"])
    assert paired[0].all(), ("parked cars that the pairing test would not pair", [names[i] for i in np.nonzero(~paired[0])[0]])
    running = np.array([not f for f in finished])
    print("long list, gap", gap, ": envs", n, "running", int(running.sum()), "manifolds per step", [int((m > 0).sum()) for m in manifolds],
          "views of running envs that leave the window, per step", [int(p[running].sum()) for p in partial])
    if touching:
        assert (manifolds[0] > 0).all(), [names[i] for i in np.nonzero(manifolds[0] == 0)[0]]
    else:
        assert (manifolds[0] == 0).all(), [names[i] for i in np.nonzero(manifolds[0])[0]]
        assert all((m[at_rest] == 0).all() for m in manifolds), "cars at rest 0.055 apart formed a manifold"
    # every pose of `stays` is in the batch; it ends at once only where the car parked beside it lands outside the playfield.  The
    # fixture has 14 such poses: at least 10 of them go on, with the views of both cars (side by side) out of the window on every step
    kept = [i for i in ed.stays if running[frames.index(i)]]
    assert set(ed.stays) <= set(frames) and len(kept) >= 10, (len(ed.stays), len(kept))
    assert all(p[running].sum() >= 20 for p in partial), "too few running envs whose views leave the window"
    assert hip.cap_hits() == (0, 0, 0, 0)
    hip.close()


def test_finished_car1_outside_the_playfield_under_car0_policy(edges):
    """(d) done_policy="car0": car 1 outside the playfield (done at the first step) stays in the world; its view -- partly outside the
    window, or far from it -- is drawn on every step, as is car 0's."""
    ed = edges
    g = ed.g
    picks = [(i, str(g["vtag"][i, 1])) for i in range(ed.F)
             if str(g["vtag"][i, 1]).split("|")[0] in ("edge", "vel", "corner") and str(g["vtag"][i, 1]).split("|")[3] in ("+0", "+30", "+200", "+330")][::3]
    picks += [(ed.tags.index("far/car1+900x"), "far|+900x|-|0")]
    assert len(picks) <= 64 and {p[1].split("|")[3] for p in picks} == {"+0", "+30", "+200", "+330", "0"}
    twins = []
    for i, _ in picks:
        cars = g["cars"][i].copy()
        cars[0] = ed.on_track[0]  # car 0 on the track, car 1 where the fixture put it
        twins.append(ed.twin(cars, g["reward"][i]))
    B = ed.batch(twins)
    n = B.n
    elapsed = np.full(n, 10, np.int64)
    hip = make_hip(ed, twins, done_policy="car0")
    hip.set_state(batch_to_hip_state(B.E, elapsed, np.zeros(n, np.int64)))
    acts = np.zeros((n, 2, 2), np.float32)
    acts[:, 0] = [0.1, 0.6]
    finished, _, partial, _ = step_and_compare(ed, hip, B, ["car1@" + p[1] for p in picks], elapsed, 5, acts, car0=True)
    assert not any(finished) and (B.E["done"][:, 1] == 1).all() and (B.E["done"][:, 0] == 0).all()
    assert all(p[:, 1].all() and not p[:, 0].any() for p in partial), "car 1's view leaves the window on every step, car 0's never"
    hip.close()


def test_single_car_env_edge_views(edges):
    """(e) players=1: the edge poses of car 0, against the oracle with its car 1 out of sight (900 units from car 0)."""
    ed = edges
    g = ed.g
    frames = [i for i in range(ed.F) if ed.group[i] in ("edge", "vel", "corner", "field")]
    twins = []
    for i in frames:
        cars = g["cars"][i].copy()
        for b in BODIES:
            for f in ("cx", "cy", "a", "vx", "vy", "w"):
                cars[1][b][f] = cars[0][b][f]
            cars[1][b]["cx"] += np.float32(900.0)
        twins.append(ed.twin(cars, g["reward"][i]))
    want = np.stack([tw.render(0, ed.map) for tw in twins])[:, None]
    hip = make_hip(ed, twins, players=1)
    hip.set_state(oracle_to_hip_state(twins))
    n = len(twins)
    got = hip.render_current().cpu().numpy().reshape(-1)[:n * 96 * 96].reshape(n, 1, 96, 96)
    bad = mismatches(got, want, [ed.tags[i] for i in frames])
    assert not bad, (len(bad), bad[:12])
    hip.close()

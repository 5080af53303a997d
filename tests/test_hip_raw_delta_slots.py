"""The delta writer's slot mapping (pong_raster_raw.hip: a group of lanes strides over one (env, view)'s dirty blocks), driven through
crl_draw_raw_delta with chosen OLD descriptors -- the buffer holds their whole draw, the record tensor holds them -- and chosen NEW
ones (the env's state, moved into its descriptors by one step that moves nothing: zero ball speed, both bats told to stay).  The
result must be byte-equal to render_descriptors(new).

What the state admits as a NEW descriptor: ball x in 0..156 (a ball past either edge scores and is served again), bats in
TOP..BOTTOM-15 (the step clamps them), scores 0..21 or 255/255 (blank); ball y is free.  An OLD descriptor is only a record, so it
takes the rest: x < 0 and x > 156, bats outside the court."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOP, BOTTOM, BAT_H = 34, 194, 15
BAT_LO, BAT_HI = TOP, BOTTOM - BAT_H  # 34 .. 179
BLANK = (0, 0, 0, 0, 255, 255)  # the library's blank frame; as a NEW descriptor a blank frame keeps bats the step leaves alone
F = dict(x=78, y=112, bl=107, br=107, sl=3, sr=5)  # a quiet frame: every case changes a few fields of it


def _fr(**kw):
    d = dict(F, **kw)
    return (d["x"], d["y"], d["bl"], d["br"], d["sl"], d["sr"])


def _cases():
    """(old, new) descriptor pairs, each (x, y, bat_l, bat_r, score_l, score_r)."""
    c = []
    # ball x over every residue of 3x mod 32 (x = 0..31), on both sides of the row, against a disjoint old rectangle
    for x in list(range(0, 32)) + list(range(140, 157)):
        c.append((_fr(x=(x + 40) % 150, y=60), _fr(x=x, y=100)))
    # the clipped edges: old balls partly or wholly outside the row
    for xo in (-5, -4, -3, -1, 157, 158, 159, 160, 161, 200, -200, 32767, -32768):
        for xn in (0, 156):
            c.append((_fr(x=xo, y=90), _fr(x=xn, y=92)))
    # ball y at, just inside and just outside the court's first and last row, as the new and as the old rectangle
    for y in (TOP - 5, TOP - 4, TOP - 3, TOP - 1, TOP, TOP + 1, BOTTOM - 5, BOTTOM - 4, BOTTOM - 3, BOTTOM - 1, BOTTOM, BOTTOM + 1, -30000, 30000):
        c.append((_fr(x=50, y=100), _fr(x=53, y=y)))
        c.append((_fr(x=50, y=y), _fr(x=53, y=100)))
        c.append((_fr(x=50, y=y), _fr(x=50, y=y + 2)))
    # old and new rectangles identical, overlapping by 1-3 rows, touching, disjoint; columns equal, shifted, apart
    for dy in range(-5, 6):
        for dx in (0, 1, 4, -6):
            c.append((_fr(x=80, y=100), _fr(x=80 + dx, y=100 + dy)))
    # the ball over each bat's column (bat pixels 16..20 and 139..143), old or new, with that bat moving under it
    for x in (12, 13, 16, 18, 20, 21, 135, 136, 139, 141, 143, 144):
        c.append((_fr(x=70, y=110, bl=100, br=100), _fr(x=x, y=103, bl=104, br=96)))
        c.append((_fr(x=x, y=111, bl=104, br=96), _fr(x=70, y=110, bl=100, br=100)))
        c.append((_fr(x=x, y=111, bl=104, br=96), _fr(x=x, y=107, bl=100, br=100)))
    # bat moves of 0, 1, 4, 8, 14, 15, 16 and 150 rows, both directions, each bat and both; old spans clamped at both court edges
    moves = []
    for d in (0, 1, 4, 8, 14, 15, 16):
        moves += [(100, 100 + d), (100 + d, 100), (BAT_LO, BAT_LO + d), (BAT_LO + d, BAT_LO), (BAT_HI, BAT_HI - d), (BAT_HI - d, BAT_HI),
                  (BAT_LO - d, BAT_LO), (BAT_HI + d, BAT_HI)]
    moves += [(20, 170), (190, 40), (0, 150), (255, 105), (BAT_LO, BAT_HI), (BAT_HI, BAT_LO), (0, BAT_LO), (255, BAT_HI), (25, BAT_HI), (19, BAT_LO)]
    for i, (o, n) in enumerate(moves):
        c.append((_fr(bl=o), _fr(bl=n)))
        c.append((_fr(br=o), _fr(br=n)))
        if i % 2 == 0:
            c.append((_fr(bl=o, br=n if BAT_LO <= n <= BAT_HI else 107), _fr(bl=n, br=o if BAT_LO <= o <= BAT_HI else 107)))
    # scores: neither side, one side, both sides; with and without court changes
    for so, sn in (((3, 5), (3, 5)), ((3, 5), (4, 5)), ((3, 5), (3, 6)), ((3, 5), (4, 6)), ((0, 0), (21, 21)), ((21, 20), (0, 0)), ((9, 10), (10, 9))):
        c.append((_fr(sl=so[0], sr=so[1]), _fr(sl=sn[0], sr=sn[1])))
        c.append((_fr(sl=so[0], sr=so[1], x=30, y=40, bl=50), _fr(sl=sn[0], sr=sn[1], x=34, y=43, bl=54)))
    # blank descriptors: old blank and new not, the reverse, both
    blank_new = _fr(sl=255, sr=255)
    c += [(BLANK, _fr()), (_fr(), blank_new), (BLANK, blank_new), (_fr(x=3, sl=255, sr=255), blank_new),
          (BLANK, _fr(x=0, y=TOP, bl=BAT_LO, br=BAT_HI, sl=21, sr=0)), (_fr(x=3, y=180), blank_new)]
    # more dirty slots than a group has lanes: two disjoint balls of two blocks a row and both bats across the court
    c += [(_fr(x=10, y=50, bl=40, br=170), _fr(x=100, y=120, bl=120, br=60)), (_fr(x=5, y=36, bl=BAT_LO, br=BAT_HI), _fr(x=150, y=188, bl=BAT_HI, br=BAT_LO)),
          (_fr(x=26, y=70, bl=0, br=255, sl=1, sr=2), _fr(x=90, y=75, bl=BAT_HI, br=BAT_LO, sl=2, sr=2))]
    # and a seeded sample of anything against anything
    rs = np.random.RandomState(5)
    for _ in range(64):
        old = (int(rs.randint(-8, 168)), int(rs.randint(20, 210)), int(rs.randint(0, 256)), int(rs.randint(0, 256)), int(rs.randint(0, 22)), int(rs.randint(0, 22)))
        new = (int(rs.randint(0, 157)), int(rs.randint(20, 210)), int(rs.randint(BAT_LO, BAT_HI + 1)), int(rs.randint(BAT_LO, BAT_HI + 1)),
               old[4] if rs.rand() < 0.7 else int(rs.randint(0, 22)), old[5] if rs.rand() < 0.7 else int(rs.randint(0, 22)))
        c.append((old, new))
    return c


CASES = _cases()


def _pack(fr):
    a = np.asarray(fr, np.int64).reshape(-1, 6)
    return ((a[:, 0] & 0xFFFF) | ((a[:, 1] & 0xFFFF) << 16) | ((a[:, 2] & 0xFF) << 32) | ((a[:, 3] & 0xFF) << 40) | ((a[:, 4] & 0xFF) << 48)
            | ((a[:, 5] & 0xFF) << 56))  # (int64: a score_r of 255 wraps into the sign bit, as the device's u64 reads it)


def _desc8(packed, dev):
    d = torch.full((8, len(packed)), -1, dtype=torch.int64, device=dev)  # (blank planes: a raw context reads planes 6 and 7 only)
    d[6] = d[7] = torch.from_numpy(packed).to(dev)
    return d


def _buffer(like, offset16):
    """A contiguous tensor of like's shape, 64-byte aligned (whole blocks) or, with offset16, 16 bytes past such a boundary inside a
    larger allocation (the single-chunk path)."""
    store = torch.empty(like.numel() + 128, dtype=torch.uint8, device=like.device)
    off = (-store.data_ptr()) % 64 + (16 if offset16 else 0)
    buf = store[off:off + like.numel()].view(like.shape)
    assert buf.data_ptr() % 64 == (16 if offset16 else 0)
    return buf


def _run(pairs, single, offset16, same_over_a5=False):
    """Draws `pairs` (one env each) through crl_draw_raw_delta with a valid record; returns nothing, asserts byte equality."""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import competitive_rl_amd as crl
    from competitive_rl_amd import _native as N

    n = len(pairs)
    env = crl.HipPongVecEnv(n, seed=1, mode="raw", single_player=single)
    try:
        env.reset()
        new = np.array([p[1] for p in pairs], np.int64)
        st = env.get_state()
        st["speed_x"], st["speed_y"] = 0.0, 0.0
        st["ball_x"], st["ball_y"], st["bat_l_y"], st["bat_r_y"] = new[:, 0], new[:, 1], new[:, 2], new[:, 3]
        st["score_l"], st["score_r"], st["num_rounds"], st["num_steps"] = new[:, 4], new[:, 5], 0, 0
        env.set_state(st)
        stay = torch.ones((n,) if single else (n, 2), dtype=torch.int32, device="cuda")
        env.step_device(stay, render=False)  # the state becomes the env's current descriptors; nothing moves
        desc_new = env.obs_descriptors()
        moved = np.nonzero(desc_new[6].cpu().numpy() != _pack(new))[0]
        assert len(moved) == 0, f"the step did not leave the chosen new descriptors of {[pairs[i][1] for i in moved[:6]]}"
        ref = env.render_descriptors(desc_new)
        old = _pack(new if same_over_a5 else [p[0] for p in pairs])
        buf = _buffer(ref, offset16)
        if same_over_a5:
            buf.fill_(0xA5)
        else:
            env.render_descriptors(_desc8(old, "cuda"), out=buf)
        rec = torch.from_numpy(old).cuda()
        L = N.load()
        rc = L.crl_draw_raw_delta(env._h, C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert torch.equal(rec, desc_new[6]), "the record does not hold the drawn descriptors"
        if same_over_a5:
            assert bool((buf == 0xA5).all()), "equal descriptors: the dirty set must be empty, yet bytes were stored"
        elif not torch.equal(buf, ref):
            bad = (buf != ref).reshape(n, buf.shape[1], -1).any(-1).nonzero()[:6].tolist()
            raise AssertionError(f"(env, view) {bad} differ from a whole draw; pairs {[pairs[e] for e, _ in bad]}")
    finally:
        env.close()


@pytest.mark.parametrize("offset16", [False, True])
@pytest.mark.parametrize("single", [False, True])
def test_every_case_equals_whole_draw(single, offset16):
    _run(CASES, single, offset16)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 130])
def test_ragged_env_counts(n, single):
    order = np.random.RandomState(n).permutation(len(CASES))[:n]
    pairs = [CASES[i] for i in order]
    _run(pairs, single, offset16=False)
    _run(pairs, single, offset16=True)


@pytest.mark.parametrize("offset16", [False, True])
@pytest.mark.parametrize("single", [False, True])
def test_equal_descriptors_store_nothing(single, offset16):
    _run(CASES, single, offset16, same_over_a5=True)

"""WHERE the raw delta writer stores (pong_raster_raw.hip, crl_draw_raw_delta).  test_hip_raw_delta_slots.py proves the drawn bytes
equal a whole draw; a store of the right bytes in the wrong place is invisible to it, because the buffer already holds the old
frame there.  Here the buffer is filled with 0xA5, and no 16-byte chunk of a frame is all 0xA5, so every stored chunk shows, and
the set of stored chunks is held between two bounds per (env, view):

  stored  <=  the dirty set of the rule (restated below from tests/test_raw_delta_rule.py), closed over the aligned 64-byte blocks
              of the buffer -- or the dirty set itself where the buffer sits 16 bytes off a 64-byte boundary (single chunks);
  stored  >=  the chunks in which whole draws of the old and of the new descriptors differ.

A second test drives the env's own two buffers through 300 real steps with points and a game end at the smallest size that
crosses a workgroup, so that the score-band and whole-frame paths run next to the court loop."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, TOP, BOTTOM, BALL, BAT_W, BAT_H, BATL_X, BATR_X = 160, 210, 34, 194, 4, 5, 15, 16, 139
ROW_CHUNKS = W * 3 // 16  # 30
BAT_LO, BAT_HI = TOP, BOTTOM - BAT_H  # 34 .. 179
BLANK = (0, 0, 0, 0, 255, 255)
F = dict(x=78, y=112, bl=107, br=107, sl=3, sr=5)  # a quiet frame: every pair changes a few fields of it


def _fr(**kw):
    d = dict(F, **kw)
    return (d["x"], d["y"], d["bl"], d["br"], d["sl"], d["sr"])


def ink_rows(atlas):
    """[r0, r1): the score-band rows where some (score_l, score_r) image has ink (crl_create's rule)"""
    rows = np.nonzero((atlas.reshape(22 * 22, TOP, W) != 255).any(axis=(0, 2)))[0]
    return (int(rows[0]), int(rows[-1]) + 1) if len(rows) else (0, 0)


def dirty_chunks(old, new, ink):
    """bool (2 views, 210 rows, 30 chunks): the chunks the rule lets the delta writer store when `old` is replaced by `new`, each
    (x, y, bat_l, bat_r, score_l, score_r) -- tests/test_raw_delta_rule.py's dirty_chunks, restated"""
    d = np.zeros((2, H, ROW_CHUNKS), bool)
    blank_o, blank_n = old[4] == 255, new[4] == 255
    if blank_o != blank_n:
        d[:] = True
        return d
    if blank_n:
        return d
    if old[4:] != new[4:]:
        d[:, ink[0]:ink[1]] = True

    def rect(r0, r1, c0, c1):  # source chunks [c0, c1] of rows [r0, r1) clamped to the court; view 1 = chunk 29 - c
        r0, r1 = max(r0, TOP), min(r1, BOTTOM)
        if r0 < r1:
            d[0, r0:r1, c0:c1 + 1] = True
            d[1, r0:r1, ROW_CHUNKS - 1 - c1:ROW_CHUNKS - c0] = True

    def ball(f):
        b0, b1 = max(3 * f[0], 0), min(3 * (f[0] + BALL), 3 * W)
        if b0 < b1:
            rect(f[1], f[1] + BALL, b0 // 16, (b1 - 1) // 16)

    if old[:2] != new[:2]:
        ball(old), ball(new)
    for i, x in ((2, BATL_X), (3, BATR_X)):
        a, b = old[i], new[i]
        if a != b:
            lo, hi = min(a, b), max(a, b)
            k = min(hi - lo, BAT_H)
            c0, c1 = 3 * x // 16, (3 * (x + BAT_W) - 1) // 16
            rect(lo, lo + k, c0, c1)
            rect(hi + BAT_H - k, hi + BAT_H, c0, c1)
    return d


def _pairs():
    """(old, new) descriptor pairs whose dirty set the rule alone keeps small; new descriptors are ones a step can leave (ball x in
    0..156, bats inside the court)"""
    c = []
    for x in (0, 5, 16, 21, 26, 140, 156):  # the ball at the row's edges, beside and over the bats' columns; the old one 40 px away
        c.append((_fr(x=x + 40 if x < 100 else x - 40, y=100), _fr(x=x, y=100)))
    # ball rows straddling TOP and BOTTOM, as the new and as the old rectangle
    c += [(_fr(x=50, y=100), _fr(x=53, y=TOP - 2)), (_fr(x=50, y=100), _fr(x=53, y=BOTTOM - 2)),
          (_fr(x=50, y=TOP - 1), _fr(x=53, y=TOP + 2)), (_fr(x=50, y=BOTTOM - 3), _fr(x=53, y=BOTTOM - 1))]
    for dy in (1, 2, 3):  # old and new ball overlapping by 3, 2, 1 rows: in the same blocks, and with the next block entered
        c.append((_fr(x=80, y=100), _fr(x=80, y=100 + dy)))
        c.append((_fr(x=80, y=100), _fr(x=84, y=100 - dy)))
    for d in (0, 1, 4, 8, 15, 16):  # each bat moved by d rows, arriving at either court edge
        c += [(_fr(bl=BAT_LO + d), _fr(bl=BAT_LO)), (_fr(bl=BAT_HI - d), _fr(bl=BAT_HI)),
              (_fr(br=BAT_LO + d), _fr(br=BAT_LO)), (_fr(br=BAT_HI - d), _fr(br=BAT_HI))]
    # the ball over each bat's column (pixels 16..20 and 139..143) while that bat moves
    c += [(_fr(x=17, y=110, bl=100), _fr(x=18, y=112, bl=104)), (_fr(x=140, y=110, br=100), _fr(x=139, y=108, br=96)),
          (_fr(x=70, y=110, bl=100), _fr(x=16, y=103, bl=104)), (_fr(x=70, y=110, br=100), _fr(x=141, y=103, br=96))]
    # a score change without and with court changes
    c += [(_fr(), _fr(sl=4)), (_fr(x=30, y=40, bl=50), _fr(x=34, y=43, bl=54, sr=6))]
    c += [(BLANK, _fr()), (_fr(), _fr())]  # blank -> drawn: the whole frame; equal descriptors: nothing
    return c


PAIRS = _pairs()
WHOLE, NOTHING = len(PAIRS) - 2, len(PAIRS) - 1
# env counts: a lone env, a half-filled wavefront, a ragged last workgroup, more than one workgroup; the first pair each starts at
# (the counts wrap round the list: 65 envs hold every pair)
COUNTS = {1: 41, 2: 0, 3: 7, 33: 11, 65: 0}


def _pack(fr):
    a = np.asarray(fr, np.int64).reshape(-1, 6)
    return ((a[:, 0] & 0xFFFF) | ((a[:, 1] & 0xFFFF) << 16) | ((a[:, 2] & 0xFF) << 32) | ((a[:, 3] & 0xFF) << 40) | ((a[:, 4] & 0xFF) << 48)
            | ((a[:, 5] & 0xFF) << 56))


def _desc8(packed, dev):
    d = torch.full((8, len(packed)), -1, dtype=torch.int64, device=dev)  # (a raw context reads planes 6 and 7 only)
    d[6] = d[7] = torch.from_numpy(packed).to(dev)
    return d


def _chunks(t, n, views):
    """(n, views, 210, 160, 3) uint8 -> (n, views, 210, 30, 16)"""
    return t.reshape(n, views, H, ROW_CHUNKS, 16)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("n", sorted(COUNTS))
def test_stores_stay_inside_the_rule(n, single, atlas):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import competitive_rl_amd as crl
    from competitive_rl_amd import _native as N

    ink = ink_rows(atlas)
    which = [(COUNTS[n] + i) % len(PAIRS) for i in range(n)]
    pairs = [PAIRS[i] for i in which]
    views = 1 if single else 2
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
        assert np.array_equal(desc_new[6].cpu().numpy(), _pack(new)), "the step did not leave the chosen new descriptors"
        old = _pack([p[0] for p in pairs])
        ref_new = env.render_descriptors(desc_new)
        ref_old = env.render_descriptors(_desc8(old, "cuda"))
        assert ref_new.shape == (n, views, H, W, 3)
        # (single bytes of the score digits' anti-aliased edges are 0xA5; a stored chunk hides only if all 16 of its bytes are)
        assert not bool(_chunks(ref_new == 0xA5, n, views).all(-1).any()), "a chunk of a frame is all 0xA5: the fill cannot mark the chunks that were not stored"
        differ = _chunks(ref_old != ref_new, n, views).any(-1).cpu().numpy()
        # the rule, and the restatement checked against whole draws before it serves as a bound
        dirty = np.stack([dirty_chunks(o, nw, ink)[:views] for o, nw in pairs])
        missed = differ & ~dirty
        assert not missed.any(), ("the rule misses a differing chunk", [pairs[e] for e in np.argwhere(missed)[:3, 0]])
        closure = np.repeat(dirty.reshape(-1, 4).any(1), 4).reshape(dirty.shape)  # blocks of 4 chunks from the buffer's start

        L = N.load()
        for offset16 in (False, True):
            store = torch.full((ref_new.numel() + 128,), 0xA5, dtype=torch.uint8, device="cuda")
            off = (-store.data_ptr()) % 64 + (16 if offset16 else 0)
            buf = store[off:off + ref_new.numel()].view(ref_new.shape)
            assert buf.data_ptr() % 64 == (16 if offset16 else 0)
            rec = torch.from_numpy(old).cuda()
            rc = L.crl_draw_raw_delta(env._h, C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            assert torch.equal(rec, desc_new[6]), "the record does not hold the drawn descriptors"
            stored_dev = ~_chunks(buf == 0xA5, n, views).all(-1)
            stored = stored_dev.cpu().numpy()
            bound = dirty if offset16 else closure
            outside = stored & ~bound
            assert not outside.any(), (f"offset16={offset16}: stores outside the rule's " + ("dirty set" if offset16 else "blocks"),
                                       [(pairs[e], (v, r, c)) for e, v, r, c in np.argwhere(outside)[:4].tolist()])
            lost = differ & ~stored
            assert not lost.any(), (f"offset16={offset16}: a differing chunk was not stored",
                                    [(pairs[e], (v, r, c)) for e, v, r, c in np.argwhere(lost)[:4].tolist()])
            assert torch.equal(_chunks(buf, n, views)[stored_dev], _chunks(ref_new, n, views)[stored_dev]), "a stored chunk does not hold the new frame's bytes"
            assert bool((store[:off] == 0xA5).all()) and bool((store[off + ref_new.numel():] == 0xA5).all()), "the slack around the buffer was stored to"
            for e, i in enumerate(which):
                if i == WHOLE:
                    assert stored[e].all(), "blank -> drawn: the whole frame must be stored"
                if i == NOTHING:
                    assert not stored[e].any(), "equal descriptors: nothing may be stored"
    finally:
        env.close()


def test_two_buffers_over_real_steps():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import competitive_rl_amd as crl

    n, steps = 67, 300
    env = crl.HipPongVecEnv(n, seed=4, mode="raw")
    try:
        env.reset()
        st = env.get_state()
        st["score_l"], st["score_r"], st["num_rounds"] = 19, 19, 19  # two points from the game's end ...
        st["score_l"][::2], st["score_r"][::2], st["num_rounds"][::2] = 20, 20, 20  # ... and one
        env.set_state(st)
        gen = torch.Generator(device="cuda").manual_seed(13)
        dones, score_changes, scores = 0, 0, None
        for t in range(steps):
            a = torch.randint(0, 4, (n, 2), generator=gen, device="cuda", dtype=torch.int32)
            buf, _, done = env.step_device(torch.where(a == 3, torch.full_like(a, 999), a))  # 0 / 1 / 2 / 999
            desc = env.obs_descriptors()
            assert torch.equal(buf, env.render_descriptors(desc)), f"step {t}: the buffer differs from a whole draw"
            now = desc[6] >> 48
            if scores is not None:
                score_changes += int((now != scores).sum())
            scores = now
            dones += int(done.sum())
        assert score_changes > 0, "no score changed inside the run: the score-band path did not run"
        assert dones > 0, "no env was reset inside the run"
    finally:
        env.close()

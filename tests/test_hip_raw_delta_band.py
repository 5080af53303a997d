"""The score-band branch of the raw delta writer (pong_raster_raw.hip): when a single point is scored it stores only the chunk columns of
the ink rows in which the band images of the old and the new pair differ (csrc/pong_band_span.h); every other score change stores the
whole ink rows.  One env per one-point transition of the shipped atlas (924), and others beside them: a game's end from (21, k) and
(k, 21), both fields changed at once, a field decreased or advanced by two, a ball move and a bat move in the step of a point, a pair
beside a blank descriptor.  Descriptors and records are injected as in tests/test_hip_raw_delta_stores.py.  Each batch is drawn into a
64-byte-aligned buffer and into one 16 bytes off, twice:

  (a) the buffer holds the whole draw of `old`: after crl_draw_raw_delta it equals the whole draw of `new`, byte for byte;
  (b) the buffer is filled with 0xA5 (no chunk of a frame is all 0xA5, so every stored chunk shows): the stored chunks are a superset
      of the chunks in which the two whole draws differ, and a subset of
        a one-point transition: ink rows x numpy's span of differing chunk columns, mirrored where the row is mirrored, closed over the
                                buffer's aligned 64-byte blocks -- on the offset buffer that set itself;
        the other pairs:        the rule of tests/test_raw_delta_rule.py (whole ink rows, the court's rectangles), closed likewise."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, TOP, BOTTOM, BALL, BAT_W, BAT_H, BATL_X, BATR_X, MIRROR_ROW = 160, 210, 34, 194, 4, 5, 15, 16, 139, 25
ROW_CHUNKS = W * 3 // 16  # 30
BLANK = (0, 0, 0, 0, 255, 255)
F = dict(x=78, y=112, bl=107, br=107, sl=3, sr=5)


def _fr(**kw):
    d = dict(F, **kw)
    return (d["x"], d["y"], d["bl"], d["br"], d["sl"], d["sr"])


def ink_rows(atlas):
    rows = np.nonzero((atlas.reshape(22 * 22, TOP, W) != 255).any(axis=(0, 2)))[0]
    return (int(rows[0]), int(rows[-1]) + 1) if len(rows) else (0, 0)


def rule_chunks(old, new, ink):
    """bool (2, 210, 30): tests/test_raw_delta_rule.py's dirty set for a pair of non-blank or blank descriptors, restated"""
    d = np.zeros((2, H, ROW_CHUNKS), bool)
    if (old[4] == 255) != (new[4] == 255):
        d[:] = True
        return d
    if new[4] == 255:
        return d
    if old[4:] != new[4:]:
        d[:, ink[0]:ink[1]] = True

    def rect(r0, r1, c0, c1):
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


def span_chunks(atlas, old, new, ink):
    """bool (2, 210, 30): ink rows x [first, last] differing chunk column of the two band images (numpy), view 1 mirrored from MIRROR_ROW on"""
    diff = np.repeat((atlas[old[4], old[5]] != atlas[new[4], new[5]]).any(0), 3)  # pixel x holds bytes 3x .. 3x + 2
    cols = np.nonzero(diff.reshape(ROW_CHUNKS, 16).any(1))[0]
    d = np.zeros((2, H, ROW_CHUNKS), bool)
    if len(cols):
        c0, c1 = int(cols[0]), int(cols[-1])
        d[0, ink[0]:ink[1], c0:c1 + 1] = True
        for r in range(ink[0], ink[1]):
            if r >= MIRROR_ROW:
                d[1, r, ROW_CHUNKS - 1 - c1:ROW_CHUNKS - c0] = True
            else:
                d[1, r, c0:c1 + 1] = True
    return d


def _batch():
    """[(old, new, one_point)]"""
    c = []
    for a in range(22):
        for b in range(22):
            if a + 1 < 22:
                c.append((_fr(sl=a, sr=b), _fr(sl=a + 1, sr=b), True))
            if b + 1 < 22:
                c.append((_fr(sl=a, sr=b), _fr(sl=a, sr=b + 1), True))
    assert len(c) == 924
    for k in (0, 7, 13, 20):  # a game's end
        c += [(_fr(sl=21, sr=k), _fr(sl=0, sr=0), False), (_fr(sl=k, sr=21), _fr(sl=0, sr=0), False)]
    for a, b in ((3, 5), (0, 0), (9, 9), (19, 1), (9, 19)):  # two fields at once
        c.append((_fr(sl=a, sr=b), _fr(sl=a + 1, sr=b + 1), False))
    c += [(_fr(sl=4, sr=5), _fr(sl=3, sr=5), False), (_fr(sl=3, sr=5), _fr(sl=3, sr=4), False), (_fr(sl=10, sr=0), _fr(sl=9, sr=0), False),
          (_fr(sl=0, sr=20), _fr(sl=0, sr=19), False), (_fr(sl=5, sr=5), _fr(sl=4, sr=6), False), (_fr(sl=1, sr=0), _fr(sl=0, sr=0), False)]  # decreased
    c += [(_fr(sl=3, sr=5), _fr(sl=5, sr=5), False), (_fr(sl=3, sr=5), _fr(sl=3, sr=7), False), (_fr(sl=9, sr=0), _fr(sl=11, sr=0), False)]  # two points
    # a ball move and a bat move in the step of a point (the serve: ball to the centre, bats to 107): bounded by the rule
    for (a, b), (a2, b2) in (((3, 5), (4, 5)), ((3, 5), (3, 6)), ((9, 9), (10, 9)), ((9, 9), (9, 10)), ((19, 0), (20, 0)), ((0, 0), (0, 1)), ((20, 20), (21, 20)),
                             ((9, 19), (9, 20))):
        c.append((_fr(x=153, y=60, bl=99, br=123, sl=a, sr=b), _fr(sl=a2, sr=b2), False))
        c.append((_fr(x=2, y=BOTTOM - 5, bl=TOP, br=BOTTOM - BAT_H, sl=a, sr=b), _fr(sl=a2, sr=b2), False))
    c += [(BLANK, _fr(sl=4), False), (_fr(sl=9, sr=9), _fr(sl=10, sr=9), True), (BLANK, _fr(sl=10, sr=9), False)]  # a pair between blank descriptors
    c += [(_fr(), _fr(), False), (_fr(x=50, y=100), _fr(x=53, y=103), False)]  # nothing; the court alone
    return c


BATCH = _batch()
# (first entry, envs): the whole batch; five envs across a workgroup of four wavefronts, the pair between two blank descriptors among them
CASES = {"all": (0, len(BATCH)), "five": (len(BATCH) - 7, 5)}


def _pack(fr):
    a = np.asarray(fr, np.int64).reshape(-1, 6)
    return ((a[:, 0] & 0xFFFF) | ((a[:, 1] & 0xFFFF) << 16) | ((a[:, 2] & 0xFF) << 32) | ((a[:, 3] & 0xFF) << 40) | ((a[:, 4] & 0xFF) << 48)
            | ((a[:, 5] & 0xFF) << 56))


def _desc8(packed, dev):
    d = torch.full((8, len(packed)), -1, dtype=torch.int64, device=dev)  # (a raw context reads planes 6 and 7 only)
    d[6] = d[7] = torch.from_numpy(packed).to(dev)
    return d


def _chunks(t, n, views):
    return t.reshape(n, views, H, ROW_CHUNKS, 16)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_band_stores(case, single, atlas):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import competitive_rl_amd as crl
    from competitive_rl_amd import _native as N

    ink = ink_rows(atlas)
    first, n = CASES[case]
    batch = BATCH[first:first + n]
    assert len(batch) == n
    views = 1 if single else 2
    env = crl.HipPongVecEnv(n, seed=1, mode="raw", single_player=single)
    try:
        env.reset()
        new = np.array([p[1] for p in batch], np.int64)
        st = env.get_state()
        st["speed_x"], st["speed_y"] = 0.0, 0.0
        st["ball_x"], st["ball_y"], st["bat_l_y"], st["bat_r_y"] = new[:, 0], new[:, 1], new[:, 2], new[:, 3]
        st["score_l"], st["score_r"], st["num_rounds"], st["num_steps"] = new[:, 4], new[:, 5], 0, 0
        env.set_state(st)
        stay = torch.ones((n,) if single else (n, 2), dtype=torch.int32, device="cuda")
        env.step_device(stay, render=False)  # the state becomes the env's current descriptors; nothing moves
        desc_new = env.obs_descriptors()
        assert np.array_equal(desc_new[6].cpu().numpy(), _pack(new)), "the step did not leave the chosen new descriptors"
        old = _pack([p[0] for p in batch])
        ref_new = env.render_descriptors(desc_new)
        ref_old = env.render_descriptors(_desc8(old, "cuda"))
        assert ref_new.shape == (n, views, H, W, 3)
        assert not bool(_chunks(ref_new == 0xA5, n, views).all(-1).any()), "a chunk of a frame is all 0xA5: the fill cannot mark the chunks that were not stored"
        differ = _chunks(ref_old != ref_new, n, views).any(-1).cpu().numpy()
        bound = np.stack([(span_chunks(atlas, o, nw, ink) if one else rule_chunks(o, nw, ink))[:views] for o, nw, one in batch])
        one = np.array([p[2] for p in batch])
        missed = differ & ~bound
        assert not missed.any(), ("the test's own bound misses a differing chunk", [batch[e] for e in np.argwhere(missed)[:3, 0]])
        closure = np.repeat(bound.reshape(-1, 4).any(1), 4).reshape(bound.shape)  # blocks of 4 chunks from the buffer's start
        print(f"{case}, {views} view(s): differing chunks per env and view {differ[one].sum() / max(one.sum() * views, 1):.1f}, "
              f"bound {bound[one].sum() / max(one.sum() * views, 1):.1f}, closed {closure[one].sum() / max(one.sum() * views, 1):.1f} (one-point pairs)")

        L = N.load()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for offset16 in (False, True):
            for fill in ("old", "a5"):
                store = torch.full((ref_new.numel() + 128,), 0xA5, dtype=torch.uint8, device="cuda")
                off = (-store.data_ptr()) % 64 + (16 if offset16 else 0)
                buf = store[off:off + ref_new.numel()].view(ref_new.shape)
                assert buf.data_ptr() % 64 == (16 if offset16 else 0)
                if fill == "old":
                    buf.copy_(ref_old)
                rec = torch.from_numpy(old).cuda()
                rc = L.crl_draw_raw_delta(env._h, C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()), 1, stream)
                assert rc == 0
                assert torch.equal(rec, desc_new[6]), "the record does not hold the drawn descriptors"
                assert bool((store[:off] == 0xA5).all()) and bool((store[off + ref_new.numel():] == 0xA5).all()), "the slack around the buffer was stored to"
                tag = f"offset16={offset16}"
                if fill == "old":  # (a)
                    wrong = _chunks(buf != ref_new, n, views).any(-1).cpu().numpy()
                    assert not wrong.any(), (f"{tag}: the buffer differs from the whole draw of the new descriptors",
                                             [(batch[e][:2], (v, r, c)) for e, v, r, c in np.argwhere(wrong)[:4].tolist()])
                    continue
                stored_dev = ~_chunks(buf == 0xA5, n, views).all(-1)  # (b)
                stored = stored_dev.cpu().numpy()
                outside = stored & ~(bound if offset16 else closure)
                assert not outside.any(), (f"{tag}: stores outside the bound", [(batch[e][:2], (v, r, c)) for e, v, r, c in np.argwhere(outside)[:4].tolist()])
                lost = differ & ~stored
                assert not lost.any(), (f"{tag}: a differing chunk was not stored", [(batch[e][:2], (v, r, c)) for e, v, r, c in np.argwhere(lost)[:4].tolist()])
                assert torch.equal(_chunks(buf, n, views)[stored_dev], _chunks(ref_new, n, views)[stored_dev]), "a stored chunk does not hold the new frame's bytes"
                print(f"  {tag}: stored chunks per env and view {stored[one].sum() / max(one.sum() * views, 1):.1f} (one-point pairs)")
    finally:
        env.close()

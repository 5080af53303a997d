"""The dirty-chunk rule of the raw delta writer (pong_raster_raw_delta_kernel, include/crl.h crl_draw_raw_delta), restated on the
host and checked against whole frames rendered by the oracle: for any pair of frame descriptors (old = what a buffer holds, new =
what is drawn), every 16-byte chunk of either view whose bytes differ must be in the set the kernel stores."""
import numpy as np

from oracle import pong_oracle as po

W, H, TOP, BOTTOM, BALL, BAT_W, BAT_H, BATL_X, BATR_X = 160, 210, 34, 194, 4, 5, 15, 16, 139
ROW_CHUNKS = W * 3 // 16  # 30


def ink_rows(atlas):
    """[r0, r1): the score-band rows where some (score_l, score_r) image has ink (crl_create's rule)"""
    rows = np.nonzero((atlas.reshape(22 * 22, TOP, W) != 255).any(axis=(0, 2)))[0]
    return (int(rows[0]), int(rows[-1]) + 1) if len(rows) else (0, 0)


def dirty_chunks(old, new, ink):
    """bool (2 views, 210 rows, 30 chunks): the chunks the delta writer stores when `old` is replaced by `new`"""
    d = np.zeros((2, H, ROW_CHUNKS), bool)
    blank_o, blank_n = old["score_l"] == 255, new["score_l"] == 255
    if blank_o != blank_n:
        d[:] = True
        return d
    if blank_n:
        return d
    if (old["score_l"], old["score_r"]) != (new["score_l"], new["score_r"]):
        d[:, ink[0]:ink[1]] = True

    def rect(r0, r1, c0, c1):  # source chunks [c0, c1] of rows [r0, r1) clamped to the court; view 1 = chunk 29 - c
        r0, r1 = max(r0, TOP), min(r1, BOTTOM)
        if r0 < r1:
            d[0, r0:r1, c0:c1 + 1] = True
            d[1, r0:r1, ROW_CHUNKS - 1 - c1:ROW_CHUNKS - c0] = True

    def ball(f):
        b0, b1 = max(3 * int(f["ball_x"]), 0), min(3 * (int(f["ball_x"]) + BALL), 3 * W)
        if b0 < b1:
            rect(int(f["ball_y"]), int(f["ball_y"]) + BALL, b0 // 16, (b1 - 1) // 16)

    if (old["ball_x"], old["ball_y"]) != (new["ball_x"], new["ball_y"]):
        ball(old), ball(new)
    for key, x in (("bat_l_y", BATL_X), ("bat_r_y", BATR_X)):
        a, b = int(old[key]), int(new[key])
        if a != b:
            lo, hi = min(a, b), max(a, b)
            k = min(hi - lo, BAT_H)
            c0, c1 = 3 * x // 16, (3 * (x + BAT_W) - 1) // 16
            rect(lo, lo + k, c0, c1)
            rect(hi + BAT_H - k, hi + BAT_H, c0, c1)
    return d


def _pairs(rs):
    """(old, new) descriptor pairs: steps of the game (ball <= 4 px across and a few px down, bats -4 / 0 / +4 at the clamps, some
    points), blank on one side or both, the ball at the walls and touching the bats, and arbitrary set_state-style jumps"""
    out = []

    def frame(x, y, bl, br, sl, sr):
        f = np.zeros((), po.FRAME_DT)
        f["ball_x"], f["ball_y"], f["bat_l_y"], f["bat_r_y"], f["score_l"], f["score_r"] = x, y, bl, br, sl, sr
        return f

    clamp = lambda y: min(max(y, TOP), BOTTOM - BAT_H)  # noqa: E731
    for i in range(600):
        x, y = int(rs.randint(0, 157)), int(rs.randint(TOP, BOTTOM - BALL + 1))
        if i % 10 == 0:
            x = (0, 156, 21, 135, 17, 139)[(i // 10) % 6]  # the walls; touching a bat; inside a bat's columns
        bl, br = (int(rs.choice([TOP, BOTTOM - BAT_H, rs.randint(TOP, BOTTOM - BAT_H + 1)])) for _ in range(2))
        sl, sr = int(rs.randint(0, 22)), int(rs.randint(0, 22))
        old = frame(x, y, bl, br, sl, sr)
        dx, dy = int(rs.randint(-4, 5)), int(rs.randint(-6, 7))
        nsl, nsr = (sl, sr) if rs.rand() < 0.7 else ((sl + 1) % 22, sr) if rs.rand() < 0.5 else (sl, (sr + 1) % 22)
        new = frame(min(max(x + dx, 0), 156), min(max(y + dy, TOP), BOTTOM - BALL), clamp(bl + 4 * int(rs.randint(-1, 2))),
                    clamp(br + 4 * int(rs.randint(-1, 2))), nsl, nsr)
        if i % 25 == 1:
            old["score_l"] = old["score_r"] = 255  # blank -> frame
        elif i % 25 == 2:
            new["score_l"] = new["score_r"] = 255  # frame -> blank
        elif i % 25 == 3:
            old["score_l"] = old["score_r"] = new["score_l"] = new["score_r"] = 255
        out.append((old, new))
    for _ in range(300):  # set_state jumps, partly outside the court
        old, new = (frame(int(rs.randint(-8, 165)), int(rs.randint(20, 200)), int(rs.randint(0, 256)), int(rs.randint(0, 256)),
                          int(rs.randint(0, 22)), int(rs.randint(0, 22))) for _ in range(2))
        if rs.rand() < 0.5:
            new["score_l"], new["score_r"] = old["score_l"], old["score_r"]
        out.append((old, new))
    return out


def test_dirty_set_covers_every_changed_chunk(atlas):
    ink = ink_rows(atlas)
    assert 0 < ink[0] < ink[1] <= TOP
    pairs = _pairs(np.random.RandomState(7))
    old = np.array([p[0] for p in pairs], po.FRAME_DT)
    new = np.array([p[1] for p in pairs], po.FRAME_DT)
    a = po.render_raw(old, atlas).reshape(len(pairs), 2, H, ROW_CHUNKS, 16)
    b = po.render_raw(new, atlas).reshape(len(pairs), 2, H, ROW_CHUNKS, 16)
    changed = (a != b).any(axis=-1)
    step_sizes = []
    for i in range(len(pairs)):
        d = dirty_chunks(old[i], new[i], ink)
        missed = changed[i] & ~d
        assert not missed.any(), (i, old[i], new[i], np.argwhere(missed)[:4])
        if i < 600 and i % 25 not in (1, 2, 3) and (old[i]["score_l"], old[i]["score_r"]) == (new[i]["score_l"], new[i]["score_r"]):
            step_sizes.append(int(d.sum()))
    # a step without a point stores at most ~48 chunks per view (ball 2 x 4 rows x 2 chunks, bats 8 rows each)
    assert step_sizes and max(step_sizes) <= 2 * 48, max(step_sizes)

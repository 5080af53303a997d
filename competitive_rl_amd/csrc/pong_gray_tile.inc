// pong_gray_tile.inc -- the body of one tile of pong_raster_gray_env_kernel, included inside the kernel's tile loop(s) (textual
// inclusion, not a function: the plain kernel's code is then exactly what it was before the stack variant existed -- wrapping the body
// in an inlined lambda changed the schedule of the template loads and cost the uint8 kernel 60 %).  The includer defines, per tile:
// view, plane, rp (ring plane), to_stack, erased (bool) and f32 (element type of this tile's destination); `continue` leaves the tile.
        uint64_t pa = words_[wave][2 * rp], pb = words_[wave][2 * rp + 1];
        pa = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(pa >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)pa);
        pb = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(pb >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)pb);
        Frame fa = unpack_frame(pa), fb = unpack_frame(pb);
        // A pair with one blank frame (the reset observation: a single frame, nothing to max with) equals
        // the pair of the frame with itself -- max(x, 0) = x -- and then takes the fast path.
        if (fa.sl == 255 && fb.sl != 255) fa = fb;
        else if (fb.sl == 255 && fa.sl != 255) fb = fa;
        const bool blank_a = fa.sl == 255, blank_b = fb.sl == 255;
        // The score rows come pre-resized from the band table when the two kept frames show
        // the same score pair, or pairs one point apart (a point scored between the two
        // max-pooled frames puts two texts under the max).  Anything else (only reachable
        // through set_state or the never-written initial buffers) is evaluated per pixel.
        bool slow = blank_a || blank_b;
        int variant = 0, sp = fa.sl * 22 + fa.sr;
        if (!slow && (fa.sl != fb.sl || fa.sr != fb.sr)) {
            const int spb = fb.sl * 22 + fb.sr;
            if (fb.sl == fa.sl + 1 && fb.sr == fa.sr) variant = 1;
            else if (fb.sl == fa.sl && fb.sr == fa.sr + 1) variant = 2;
            else if (fa.sl == fb.sl + 1 && fa.sr == fb.sr) variant = 1, sp = spb;
            else if (fa.sl == fb.sl && fa.sr == fb.sr + 1) variant = 2, sp = spb;
            else slow = true;
        }
        {
            const int64_t tile = to_stack ? env * ks + plane : (env * q.views + view) * K + plane;
            uint8_t *__restrict__ dst = to_stack ? sk.out : obs;
            uint4 *__restrict__ out = reinterpret_cast<uint4 *>(dst + tile * (int64_t)RR);
            uint32_t *__restrict__ out32 = reinterpret_cast<uint32_t *>(dst + tile * (int64_t)RR);
            float4 *__restrict__ outf = reinterpret_cast<float4 *>(dst) + tile * (int64_t)(RR >> 2);  // F32: RR % 4 == 0
            if ((blank_a && blank_b) || erased) {  // plane erased by a done (FrameStackTensor mask), or older than the bound stack's reset()
                if (f32)
                    for (int w = lane; w < (RR >> 2); w += 64) outf[w] = make_float4(0.f, 0.f, 0.f, 0.f);
                else if (vec16)
                    for (int c = lane; c < chunks; c += 64) out[c] = make_uint4(0, 0, 0, 0);
                else
                    for (int w = lane; w < (RR >> 2); w += 64) out32[w] = 0u;
                continue;
            }
            // ---- 1. template loads into registers (L2); the box arithmetic and the row / column
            //         words below overlap their latency, the LDS tile is filled afterwards
            const uint4 *__restrict__ band4 =
                reinterpret_cast<const uint4 *>(q.band) + (int64_t)((slow ? 0 : (variant * 484 + sp)) * 2 + view) * bb;
            uint4 tv[TI];
#pragma unroll
            for (int it = 0; it < TI; it++) {
                const int c = lane + 64 * it;
                tv[it] = make_uint4(0, 0, 0, 0);
                if (c < bb) tv[it] = band4[c];
                else if (c < chunks && (c < zc0 || c >= zc1)) tv[it] = rest4[c];
            }
            // ---- 2. patch: boxes of the six rectangles in view coordinates (scalar)
            const bool m = view == 1;
            Rects rc;
            rc.ax = blank_a ? -1000 : (m ? CRL_PONG_W - fa.x - CRL_PONG_BALL : fa.x), rc.ay = blank_a ? -1000 : fa.y;
            rc.bx = blank_b ? -1000 : (m ? CRL_PONG_W - fb.x - CRL_PONG_BALL : fb.x), rc.by = blank_b ? -1000 : fb.y;
            rc.la = blank_a ? -1000 : (m ? fa.br : fa.bl), rc.ra = blank_a ? -1000 : (m ? fa.bl : fa.br);
            rc.lb = blank_b ? -1000 : (m ? fb.br : fb.bl), rc.rb = blank_b ? -1000 : (m ? fb.bl : fb.br);
            Box bx[6];
            {
#ifndef CRL_GRAY_BOX_BRANCHY  // (round 6: the boxes without control flow -- 84 x 84: K = 1 219 -> 214.5 us, K = 4 748 -> 742; 42 x 42: +- 0)
                auto box = [&](bool none, int c0, int c1, int r0, int r1) { return rect_box_lds_nb(tabs, q.t, none, c0, c1, r0, r1); };
#else
                auto box = [&](bool none, int c0, int c1, int r0, int r1) {
                    const Box b = {0, 0, 0, 0};
                    return none ? b : rect_box_lds(tabs, q.t, c0, c1, r0, r1);
                };
#endif
                const bool same_ball = rc.ax == rc.bx && rc.ay == rc.by;
                bx[0] = box(blank_a, rc.ax, rc.ax + CRL_PONG_BALL, max(rc.ay, CRL_PONG_TOP), min(rc.ay + CRL_PONG_BALL, CRL_PONG_BOTTOM));
                bx[1] = box(blank_a, CRL_PONG_BATL_X, CRL_PONG_BATL_X + CRL_PONG_BAT_W, rc.la, rc.la + CRL_PONG_BAT_H);
                bx[2] = box(blank_a, CRL_PONG_BATR_X, CRL_PONG_BATR_X + CRL_PONG_BAT_W, rc.ra, rc.ra + CRL_PONG_BAT_H);
                bx[3] = box(blank_b || same_ball, rc.bx, rc.bx + CRL_PONG_BALL, max(rc.by, CRL_PONG_TOP), min(rc.by + CRL_PONG_BALL, CRL_PONG_BOTTOM));
                bx[4] = box(blank_b || rc.la == rc.lb, CRL_PONG_BATL_X, CRL_PONG_BATL_X + CRL_PONG_BAT_W, rc.lb, rc.lb + CRL_PONG_BAT_H);
                bx[5] = box(blank_b || rc.ra == rc.rb, CRL_PONG_BATR_X, CRL_PONG_BATR_X + CRL_PONG_BAT_W, rc.rb, rc.rb + CRL_PONG_BAT_H);
            }
            int pre[7];
            float rw[6];
            pre[0] = slow ? q.band_rows * R : 0;  // slow path: evaluate every pixel of the score rows
            int ymin = R, ymax = 0, xmin = R, xmax = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                pre[i + 1] = pre[i] + bx[i].w * bx[i].h, rw[i] = 1.0f / (float)max(bx[i].w, 1);
                if (bx[i].w * bx[i].h > 0) {
                    ymin = min(ymin, bx[i].y0), ymax = max(ymax, bx[i].y0 + bx[i].h);
                    xmin = min(xmin, bx[i].x0), xmax = max(xmax, bx[i].x0 + bx[i].w);
                }
            }
            const int total = pre[6];
            uint32_t *rowpack = rowpack_[wave], *colpack = colpack_[wave];
            if (fast_ok) {
                for (int dy = ymin + lane; dy < ymax; dy += 64) rowpack[dy] = row_pack<MAXT>(tabs, q.t, rc, dy);
                for (int dx = xmin + lane; dx < xmax; dx += 64) colpack[dx] = col_pack<MAXT>(tabs, q.t, rc, dx);
            }
#pragma unroll
            for (int it = 0; it < TI; it++)
                if (lane + 64 * it < chunks) tl4[lane + 64 * it] = tv[it];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            for (int p = lane; p < total; p += 64) {
                int dy, dx;
                const bool band_px = p < pre[0];
                if (band_px) {
                    dy = p / R, dx = p - dy * R;
                } else {
                    // select the box without dynamic register indexing
                    int x0 = bx[0].x0, y0 = bx[0].y0, w = bx[0].w, base = pre[0];
                    float r = rw[0];
#pragma unroll
                    for (int k = 1; k < 6; k++)
                        if (p >= pre[k]) x0 = bx[k].x0, y0 = bx[k].y0, w = bx[k].w, base = pre[k], r = rw[k];
                    const int o = p - base;
                    const int yy = (int)(((float)o + 0.5f) * r);  // o / w, exact for these sizes
                    dy = y0 + yy, dx = x0 + (o - yy * w);
                }
                uint8_t v;
                if (band_px || !fast_ok) v = eval_pixel(g, fa, fb, view, dy, dx);
                else v = eval_sep<MAXT>(tabs, q.t, R, rowpack[dy], colpack[dx], dy, dx);
                tl[dy * R + dx] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            // ---- 3. stream the tile out
            if (f32) {
                const uint32_t *tl32 = reinterpret_cast<const uint32_t *>(tl);
                constexpr int NG = TI * 4;  // 256-pixel groups of the LDS tile
                constexpr int EP = CRL_F32_EPI < NG ? CRL_F32_EPI : NG;  // groups per batch: all LDS reads of a batch first, then its stores
#pragma unroll
                for (int g0 = 0; g0 < NG; g0 += EP) {
                    uint32_t px[EP];
#pragma unroll
                    for (int gi = 0; gi < EP; gi++) px[gi] = tl32[min(lane + 64 * (g0 + gi), (RR >> 2) - 1)];
#pragma unroll
                    for (int gi = 0; gi < EP; gi++)
                        if (g0 + gi < NG && lane + 64 * (g0 + gi) < (RR >> 2))
                            outf[lane + 64 * (g0 + gi)] = make_float4((float)(px[gi] & 255u), (float)((px[gi] >> 8) & 255u), (float)((px[gi] >> 16) & 255u),
                                                                      (float)(px[gi] >> 24));
                }
            } else if (vec16) {
                // all LDS reads first, then the stores (a rolled loop would wait for every read in turn)
                uint4 ov[TI];
#pragma unroll
                for (int it = 0; it < TI; it++) ov[it] = tl4[min(lane + 64 * it, chunks - 1)];
#pragma unroll
                for (int it = 0; it < TI; it++)
                    if (lane + 64 * it < chunks) out[lane + 64 * it] = ov[it];
            } else {
                const uint32_t *tl32 = reinterpret_cast<const uint32_t *>(tl);
                for (int w = lane; w < (RR >> 2); w += 64) out32[w] = tl32[w];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }

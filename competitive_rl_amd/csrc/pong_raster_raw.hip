// pong_raster_raw.hip -- raw cPongDouble observation writer: (N, 2, 210, 160, 3) uint8.
//
// Restates PongGame.draw + Scoreboard.draw + _surface_to_img + the second agent's
// mirrored view (reference pong/base_pong_env.py:259-266, 72-74, 149-155) as an
// ANALYTIC pixel function of the 8-byte frame descriptor -- nothing is read back,
// nothing is copied between views.
//
// Roofline: pure HBM store stream, 201 600 B per env-step, no reuse.  The env's two frames
// are 12 600 16-byte chunks; a chunk's 16 bytes are built in registers:
//   rows <34  : white, or (ink rows only) a 16-byte load from the RGB-expanded score
//               band of this (score_l, score_r) -- L2/MALL resident, ~8 MB total;
//   rows 34-193: 16-bit coverage mask of ball/bat rectangles -> 4 dwords of 0x00/0xFF;
//   rows >=194: white.
// Agent 1's view is rows >= 25 mirrored; since every pixel is achromatic (R=G=B) a
// mirrored chunk is the byte-reversed chunk (29 - c) of the unmirrored row.
// Three work splits: pong_raster_raw_sweep_kernel (production: address-linear, a thread's four chunks a whole grid
// apart), pong_raster_raw_linear_kernel (address-linear, a workgroup's chunks contiguous; CRL_RAW_SWEEP=0) and the
// original one workgroup per env (thread t writes chunks t, t+256, ...; CRL_RAW_SWEEP=0 CRL_RAW_LINEAR=0), kept for A/B.
#include <stdlib.h>

#include "crl_internal.h"
#include "pong_device.h"

namespace crl {

static constexpr int kRowBytes = CRL_PONG_W * 3;            // 480
static constexpr int kRowChunks = kRowBytes / 16;           // 30
static constexpr int kFrameChunks = CRL_PONG_H * kRowChunks;  // 6300

__device__ inline uint32_t nibble_to_bytes(uint32_t nib) {
    // bit k of nib -> byte k = 0xFF
    return ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;
}

__device__ inline uint32_t span_bits(int a, int b) {
    // bits [a, b) of a 16-bit chunk mask, a/b in chunk-local byte coordinates (any int)
    a = max(a, 0), b = min(b, 16);
    return a < b ? (((1u << b) - 1u) & ~((1u << a) - 1u)) : 0u;
}

__device__ inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// The 16 bytes of chunk q (0 .. views * kFrameChunks - 1) of one env's frames: THE pixel function of this file, shared by
// the three work splits below.  dbg: 1 = constants only, 2 = no score-band loads (profiling).
__device__ __forceinline__ uint4 raw_chunk(const Frame &f, int q, const uint4 *__restrict__ atlas_rgb, int ink_row0, int ink_row1, int dbg) {
    const bool blank = f.sl == 255;
    const uint32_t bg = blank ? 0u : 0xFFFFFFFFu;
    const int view = q >= kFrameChunks;
    const int c = q - view * kFrameChunks;
    const int row = c / kRowChunks;
    const int cc = c - row * kRowChunks;
    const bool mirror = view && row >= CRL_PONG_MIRROR_ROW;
    const int sc = mirror ? (kRowChunks - 1 - cc) : cc;  // source chunk in the unmirrored row
    uint4 v = make_uint4(bg, bg, bg, bg);
    if (!blank && !(dbg & 1)) {
        if (row < CRL_PONG_TOP) {
            if (row >= ink_row0 && row < ink_row1 && !(dbg & 2)) v = atlas_rgb[(int64_t)((f.sl * 22 + f.sr) * CRL_PONG_TOP + row) * kRowChunks + sc];
        } else if (row < CRL_PONG_BOTTOM) {
            const int lo = sc * 16;
            uint32_t m = 0;
            if (row >= f.y && row < f.y + CRL_PONG_BALL) m |= span_bits(3 * f.x - lo, 3 * (f.x + CRL_PONG_BALL) - lo);
            if (row >= f.bl && row < f.bl + CRL_PONG_BAT_H)
                m |= span_bits(3 * CRL_PONG_BATL_X - lo, 3 * (CRL_PONG_BATL_X + CRL_PONG_BAT_W) - lo);
            if (row >= f.br && row < f.br + CRL_PONG_BAT_H)
                m |= span_bits(3 * CRL_PONG_BATR_X - lo, 3 * (CRL_PONG_BATR_X + CRL_PONG_BAT_W) - lo);
            v = make_uint4(nibble_to_bytes(m & 15u), nibble_to_bytes((m >> 4) & 15u), nibble_to_bytes((m >> 8) & 15u),
                           nibble_to_bytes((m >> 12) & 15u));
        }
        if (mirror) v = make_uint4(bswap32(v.w), bswap32(v.z), bswap32(v.y), bswap32(v.x));
    }
    return v;
}

// of two neighbouring envs' descriptors, the one chunk index q (relative to the first) falls into
__device__ __forceinline__ Frame pick_frame(const Frame &f0, const Frame &f1, bool second) {
    Frame f;
    f.x = second ? f1.x : f0.x, f.y = second ? f1.y : f0.y, f.bl = second ? f1.bl : f0.bl, f.br = second ? f1.br : f0.br;
    f.sl = second ? f1.sl : f0.sl, f.sr = second ? f1.sr : f0.sr;
    return f;
}

#ifdef CRL_ABLATION  // superseded writers (one workgroup per env; workgroup-contiguous): profiling build only, CRL_RAW_SWEEP=0
__global__ __launch_bounds__(256) void pong_raster_raw_kernel(const uint64_t *__restrict__ frames,
                                                              const uint4 *__restrict__ atlas_rgb, int ink_row0,
                                                              int ink_row1, uint4 *__restrict__ obs, int views, int dbg) {
    const int64_t env = blockIdx.x;
    const uint64_t packed = frames[env];  // wave-uniform -> scalar load
    const Frame f = unpack_frame(packed);
    uint4 *__restrict__ out = obs + env * (int64_t)(views * kFrameChunks);
    for (int q = threadIdx.x; q < views * kFrameChunks; q += 256) out[q] = raw_chunk(f, q, atlas_rgb, ink_row0, ink_row1, dbg);
}

// Address-linear kernel, workgroup-contiguous (production until the sweep variant below): workgroup b writes chunks [b * 512, (b + 1) * 512) of
// the WHOLE output tensor -- two 16-byte chunks per thread, 8 KiB per workgroup -- whichever envs
// they belong to (at most two).  Measured on MI355X at 65 536 envs (13.2 GB per launch):
//   one workgroup per env, 49 chunks per thread            2 250-2 300 us  (5.8 TB/s)
//   address-linear, 1 / 2 / 4 / 8 chunks per thread    2 550 / 2 030 / 2 120 / 2 180 us
//   torch.Tensor.fill_ of the same bytes (ceiling)           1 915 us      (6.9 TB/s)
// With one workgroup per env the ~2 000 resident workgroups write 2 000 separate streams 201 600 B
// apart, which DRAM sees as that many open pages; here the resident workgroups cover one moving
// 16 MB window of the tensor, like a plain fill.  One chunk per thread is bound by wave launch
// plus the frame-descriptor load in front of every wave; more than two widen the window again.
// The pixel arithmetic itself is off the critical path (removing it changes nothing).
template <int ITERS, int THREADS, int VIEWS>
__global__ __launch_bounds__(THREADS) void pong_raster_raw_linear_kernel(const uint64_t *__restrict__ frames,
                                                                         const uint4 *__restrict__ atlas_rgb, int ink_row0,
                                                                         int ink_row1, uint4 *__restrict__ obs, int views, int64_t n,
                                                                         int dbg) {
    constexpr int per_env = VIEWS * kFrameChunks;
    const int64_t g0 = (int64_t)blockIdx.x * (THREADS * ITERS);
    const int64_t total = n * per_env;
    const int64_t e0 = g0 / per_env;  // first env of this span; the span is shorter than one env
    const int64_t e1 = e0 + 1 < n ? e0 + 1 : e0;
    const Frame f0 = unpack_frame(frames[e0]), f1 = unpack_frame(frames[e1]);  // uniform -> scalar loads
    const int q0 = (int)(g0 - e0 * per_env);
#pragma unroll
    for (int i = 0; i < ITERS; i++) {
        const int64_t g = g0 + i * THREADS + threadIdx.x;
        if (g >= total) break;
        int q = q0 + i * THREADS + (int)threadIdx.x;
        const bool second = q >= per_env;
        q -= second ? per_env : 0;
        obs[g] = raw_chunk(pick_frame(f0, f1, second), q, atlas_rgb, ink_row0, ink_row1, dbg);
    }
}

#endif  // CRL_ABLATION

// Sweep variant of the address-linear kernel: thread t of workgroup b writes chunks b * 256 + t + i * (gridDim.x * 256),
// i = 0 .. ITERS-1 -- every "round" i of the whole chip is one dense linear sweep over 1/ITERS of the tensor.  Pure-store
// probes (tools/store_order_probe.hip): a wavefront that walks through a private contiguous span makes the chip write a
// comb (one tooth per resident wavefront) and loses 8-20 % of the fill rate; stores a whole grid apart do not, however
// many a wavefront issues.  Per round a workgroup's 4 KB block touches at most two envs (two scalar descriptor loads).
template <int ITERS, int VIEWS>
__global__ __launch_bounds__(256) void pong_raster_raw_sweep_kernel(const uint64_t *__restrict__ frames, const uint4 *__restrict__ atlas_rgb,
                                                                    int ink_row0, int ink_row1, uint4 *__restrict__ obs, int64_t n, int dbg) {
    constexpr int per_env = VIEWS * kFrameChunks;
    const int64_t total = n * per_env;
    const int64_t stride = (int64_t)gridDim.x * 256;
    Frame f0[ITERS], f1[ITERS];
    int q0[ITERS];
#pragma unroll
    for (int i = 0; i < ITERS; i++) {
        int64_t g0 = (int64_t)blockIdx.x * 256 + i * stride;
        g0 = g0 < total ? g0 : total - 1;
        const int64_t e0 = g0 / per_env;
        const int64_t e1 = e0 + 1 < n ? e0 + 1 : e0;
        f0[i] = unpack_frame(frames[e0]), f1[i] = unpack_frame(frames[e1]);  // uniform -> scalar loads, all issued up front
        q0[i] = (int)(g0 - e0 * per_env);
    }
#pragma unroll
    for (int i = 0; i < ITERS; i++) {
        const int64_t g = (int64_t)blockIdx.x * 256 + i * stride + threadIdx.x;
        if (g >= total) break;
        int q = q0[i] + (int)threadIdx.x;
        const bool second = q >= per_env;
        q -= second ? per_env : 0;
        obs[g] = raw_chunk(pick_frame(f0[i], f1[i], second), q, atlas_rgb, ink_row0, ink_row1, dbg);
    }
}

// Delta writer: the buffer an env draws into holds the frame of an earlier descriptor `drawn[env]` (the caller's record, see
// crl_draw_raw_delta), and a frame is a pure function of its descriptor, so only the chunks whose bytes can differ between the
// two descriptors are stored -- each still built by raw_chunk(), so the result is the full draw's, bit for bit.  Dirty set (a
// superset of the differing chunks for ANY pair of descriptors):
//   exactly one descriptor blank ..................... the whole frame;
//   both blank ....................................... nothing;
//   otherwise (sl, sr) differ ........................ every chunk of the score-band ink rows [ink_row0, ink_row1);
//            and in rows TOP..BOTTOM-1, per object:   ball: the chunks of both 4 x 4 rectangles;
//                                                     bat:  its chunk column in the rows of the symmetric difference of its old
//                                                           and new 15-row spans (<= 8 rows for a 4-px move).
// A pixel of the court is white iff the ball or a bat covers it, so a pixel that changes lies in the symmetric difference of
// some object's two rectangles; rows outside the court and the ink rows are white in every non-blank frame.
// Mapping: a group of L lanes owns one (env, view) and strides over that view's dirty slots, so the stores of one instruction
// go side by side into one frame instead of into 64 frames 201 600 B apart.  The dirty set is a list of six rectangles (new
// ball, old ball, two row spans per bat) in output-chunk coordinates; slot s of the running sum maps back to (rectangle, row,
// block, chunk of the block) with the chunk fastest, then the block, then the row.  A slot is one 16-byte chunk of an aligned
// block of G chunks (production G = 4: a whole 64-byte memory request from four adjacent lanes), all of them built from the NEW
// descriptor: the chunks of a block that are not dirty are rewritten with the bytes they hold.  Slots of the old ball's rectangle that the
// new one covers are stored once.  Two lanes may still store the same block (the ball over a bat's column): both write the new
// frame's bytes, so the race is benign.  Whole frames and score bands (a few envs per step) are strided over by the same lanes.
// The record is read and then written by the env's own wavefront (behind a barrier where the env's two views are two wavefronts).
// Measured on MI355X at 65 536 envs, two views, the launch inside the bench's event brackets (profiles/r08_raw_summary.txt):
//   one lane per env, 16-byte chunks (round 7) ........ 164 us   3.5 M memory write requests, 95 % of them 32-byte with a mask
//   L = 32, G = 1 / G = 2 (whole 32-byte sectors) ..... 168 / 164 us   (the requests neither merge nor get cheaper)
//   L = 32, G = 4 (whole 64-byte blocks) ..............  97 us   (88.6 against the round-7 mapping's 151 on a second box)
//   L = 16 / 64, G = 4 ................................ 101 / 108 us on that second box
// The cost was the partial memory request, not the byte count (G = 4 writes 198 MB against 118.7) and not the lane order.
static constexpr int kBatLc0 = 3 * CRL_PONG_BATL_X / 16, kBatLc1 = (3 * (CRL_PONG_BATL_X + CRL_PONG_BAT_W) - 1) / 16;
static constexpr int kBatRc0 = 3 * CRL_PONG_BATR_X / 16, kBatRc1 = (3 * (CRL_PONG_BATR_X + CRL_PONG_BAT_W) - 1) / 16;

// rows [r0, r0 + nr) of the court x output chunks [o0, o1] of each row (at most two), the view's mirroring applied
struct DeltaRect {
    int r0, nr, o0, o1;
};

// (rows [r0, r1) clamped to the court) x (source chunks [c0, c1]): the mirrored view's chunk of source chunk c is 29 - c
__device__ __forceinline__ DeltaRect delta_rect(int view, int r0, int r1, int c0, int c1) {
    r0 = max(r0, CRL_PONG_TOP), r1 = min(r1, CRL_PONG_BOTTOM);
    const bool mirror = view != 0;  // (court rows are all >= CRL_PONG_MIRROR_ROW)
    DeltaRect r;
    r.r0 = r0, r.nr = max(r1 - r0, 0);
    r.o0 = mirror ? kRowChunks - 1 - c1 : c0, r.o1 = mirror ? kRowChunks - 1 - c0 : c1;
    return r;
}

// the rows of the symmetric difference of [a, a + h) and [b, b + h): [lo, lo + k) and [hi + h - k, hi + h), k = min(|a - b|, h)
__device__ __forceinline__ void delta_bat(DeltaRect *r, int view, int a, int b, int c0, int c1) {
    const int lo = min(a, b), hi = max(a, b), k = min(hi - lo, CRL_PONG_BAT_H);
    r[0] = delta_rect(view, lo, lo + k, c0, c1);
    r[1] = delta_rect(view, hi + CRL_PONG_BAT_H - k, hi + CRL_PONG_BAT_H, c0, c1);
}

__device__ __forceinline__ DeltaRect delta_ball(int view, const Frame &g, bool moved) {
    const int b0 = max(3 * g.x, 0), b1 = min(3 * (g.x + CRL_PONG_BALL), kRowBytes);  // bytes of the row the ball covers
    DeltaRect r = delta_rect(view, g.y, g.y + CRL_PONG_BALL, b0 / 16, (max(b1, 1) - 1) / 16);
    if (!moved || b0 >= b1) r.nr = 0;
    return r;
}

// blocks of G = 1 << SH chunks a rectangle's row touches: the block of its first chunk counts from the view's first chunk, and a
// row starts 0 or 2 chunks into a 4-chunk block, so the larger of the two counts (slots past a row's last block store nothing)
template <int SH>
__device__ __forceinline__ int delta_blocks(const DeltaRect &r) {
    const int n0 = (r.o1 >> SH) - (r.o0 >> SH) + 1, n2 = ((r.o1 + 2) >> SH) - ((r.o0 + 2) >> SH) + 1;
    return max(n0, n2);
}

template <int VIEWS, int L, int G>
__global__ __launch_bounds__(256) void pong_raster_raw_delta_kernel(const uint64_t *__restrict__ frames, uint64_t *__restrict__ drawn,
                                                                    const uint4 *__restrict__ atlas_rgb, int ink_row0, int ink_row1,
                                                                    uint4 *__restrict__ obs, int64_t n) {
    static_assert((L == 16 || L == 32 || L == 64) && (G == 1 || G == 2 || G == 4) && (VIEWS == 1 || VIEWS == 2), "");
    constexpr int per_env = VIEWS * kFrameChunks, SH = G == 4 ? 2 : G == 2 ? 1 : 0;
    constexpr int GW = 64 / L;  // groups per wavefront
    const int64_t gw = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);  // this wavefront, of the grid
    const int lane = (int)threadIdx.x & (L - 1);
    int64_t env;
    int view;
    if constexpr (GW >= VIEWS) {  // a wavefront holds GW / VIEWS whole envs: one env -> uniform descriptor loads
        constexpr int E = GW / VIEWS;
        const int sub = ((int)threadIdx.x & 63) / L;
        env = gw * E + (E > 1 ? sub / VIEWS : 0), view = sub % VIEWS;
    } else {  // L = 64, two views: an env is two wavefronts of one workgroup
        env = gw / VIEWS, view = (int)(gw % VIEWS);
    }
    const bool valid = env < n;
    const uint64_t pn = valid ? frames[env] : kBlankFrame, po = valid ? drawn[env] : kBlankFrame;
    if constexpr (GW < VIEWS) __syncthreads();  // both wavefronts of the env have read its record
    if (valid && view == 0 && lane == 0) drawn[env] = pn;
    const Frame f = unpack_frame(pn), g = unpack_frame(po);
    const bool blank_n = f.sl == 255, blank_o = g.sl == 255;
    if (!valid || (blank_n && blank_o)) return;  // (two blank frames are equal)
    uint4 *__restrict__ out = obs + env * per_env;
    const int q_view = view * kFrameChunks;
    if (blank_n != blank_o) {  // the whole frame
        for (int c = lane; c < kFrameChunks; c += L) out[q_view + c] = raw_chunk(f, q_view + c, atlas_rgb, ink_row0, ink_row1, 0);
        return;
    }
    if ((f.sl != g.sl || f.sr != g.sr) && ink_row1 > ink_row0) {  // the score band's ink rows
        const int c0 = q_view + ink_row0 * kRowChunks, cn = (ink_row1 - ink_row0) * kRowChunks;
        for (int c = lane; c < cn; c += L) out[c0 + c] = raw_chunk(f, c0 + c, atlas_rgb, ink_row0, ink_row1, 0);
    }

    DeltaRect r[6];
    const bool moved = f.x != g.x || f.y != g.y;
    r[0] = delta_ball(view, f, moved), r[1] = delta_ball(view, g, moved);
    delta_bat(r + 2, view, g.bl, f.bl, kBatLc0, kBatLc1);
    delta_bat(r + 4, view, g.br, f.br, kBatRc0, kBatRc1);
    int nb[6], end[6], S = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) nb[i] = delta_blocks<SH>(r[i]), S += r[i].nr * nb[i] * G, end[i] = S;
    for (int s = lane; s < S; s += L) {
        int k = 0;  // the rectangle slot s falls into, and its index there
#pragma unroll
        for (int i = 0; i < 5; i++) k += s >= end[i];
        DeltaRect rc = r[0];
        int t = s, nbk = nb[0];
#pragma unroll
        for (int i = 1; i < 6; i++)
            if (k == i) rc = r[i], t = s - end[i - 1], nbk = nb[i];
        const int j = t & (G - 1), u = t >> SH;                             // chunk of the block; (row, block) of the rectangle
        const int dr = nbk == 2 ? u >> 1 : u, b = nbk == 2 ? u & 1 : 0;  // (a rectangle's row touches one or two blocks)
        const int q_row = q_view + (rc.r0 + dr) * kRowChunks;
        const int blk = ((q_row + rc.o0) >> SH) + b;
        if (blk > ((q_row + rc.o1) >> SH)) continue;
        if (k == 1 && dr + rc.r0 >= r[0].r0 && dr + rc.r0 < r[0].r0 + r[0].nr && blk >= ((q_row + r[0].o0) >> SH) &&
            blk <= ((q_row + r[0].o1) >> SH))
            continue;  // the new ball's rectangle stores this block
        const int q = (blk << SH) + j;
        out[q] = raw_chunk(f, q, atlas_rgb, ink_row0, ink_row1, 0);
    }
}

#ifdef CRL_ABLATION  // superseded mapping (one lane per env, one wavefront per (view, object) of 64 envs): profiling build only, CRL_RAW_DELTA_LANES=1
__device__ __forceinline__ void delta_store(uint4 *__restrict__ out, const Frame &f, const DeltaRect &r, int view, const uint4 *__restrict__ atlas_rgb,
                                            int ink_row0, int ink_row1) {
    for (int row = r.r0; row < r.r0 + r.nr; row++)
        for (int o = r.o0; o <= r.o1; o++) {
            const int q = view * kFrameChunks + row * kRowChunks + o;
            out[q] = raw_chunk(f, q, atlas_rgb, ink_row0, ink_row1, 0);
        }
}

template <int VIEWS>
__global__ __launch_bounds__(64 * 3 * VIEWS) void pong_raster_raw_delta_lanes_kernel(const uint64_t *__restrict__ frames, uint64_t *__restrict__ drawn,
                                                                                   const uint4 *__restrict__ atlas_rgb, int ink_row0, int ink_row1,
                                                                                   uint4 *__restrict__ obs, int64_t n) {
    constexpr int per_env = VIEWS * kFrameChunks;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int view = wave / 3, obj = wave - 3 * view;  // obj: 0 ball, 1 left bat, 2 right bat
    const int64_t env = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = env < n;
    const uint64_t pn = valid ? frames[env] : kBlankFrame, po = valid ? drawn[env] : kBlankFrame;
    __syncthreads();  // every wavefront has read drawn[] of this workgroup's envs
    if (wave == 0 && valid) drawn[env] = pn;
    const Frame f = unpack_frame(pn), g = unpack_frame(po);
    const bool blank_n = f.sl == 255, blank_o = g.sl == 255;
    const bool whole = blank_n != blank_o;
    const bool band = !blank_n && !blank_o && (f.sl != g.sl || f.sr != g.sr) && ink_row1 > ink_row0;

    // cooperative part: whole frames, then score bands, of the flagged envs (every wavefront of the view sees the same flags)
    const int t = obj * 64 + lane;  // 0 .. 191 within the view
    for (uint64_t m = __ballot(whole); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const int64_t e = (int64_t)blockIdx.x * 64 + l;
        const Frame fe = unpack_frame(frames[e]);
        uint4 *__restrict__ out = obs + e * per_env;
        for (int c = t; c < kFrameChunks; c += 192) out[view * kFrameChunks + c] = raw_chunk(fe, view * kFrameChunks + c, atlas_rgb, ink_row0, ink_row1, 0);
    }
    for (uint64_t m = __ballot(band); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const int64_t e = (int64_t)blockIdx.x * 64 + l;
        const Frame fe = unpack_frame(frames[e]);
        uint4 *__restrict__ out = obs + e * per_env;
        const int c0 = view * kFrameChunks + ink_row0 * kRowChunks, cn = (ink_row1 - ink_row0) * kRowChunks;
        for (int c = t; c < cn; c += 192) out[c0 + c] = raw_chunk(fe, c0 + c, atlas_rgb, ink_row0, ink_row1, 0);
    }
    if (!valid || whole || blank_n) return;  // (a whole frame is drawn above; two blank frames are equal)

    // per-lane part: this env's object in this view
    uint4 *__restrict__ out = obs + env * per_env;
    DeltaRect r[2];
    if (obj == 0) {
        const bool moved = f.x != g.x || f.y != g.y;
        r[0] = delta_ball(view, g, moved), r[1] = delta_ball(view, f, moved);
    } else if (obj == 1) {
        delta_bat(r, view, g.bl, f.bl, kBatLc0, kBatLc1);
    } else {
        delta_bat(r, view, g.br, f.br, kBatRc0, kBatRc1);
    }
    delta_store(out, f, r[0], view, atlas_rgb, ink_row0, ink_row1);
    delta_store(out, f, r[1], view, atlas_rgb, ink_row0, ink_row1);
}
#endif  // CRL_ABLATION

static constexpr int kDeltaL = 32, kDeltaG = 4;  // production: lanes per (env, view); chunks per block (4: whole 64-byte memory requests)

void launch_pong_raster_raw_delta(const uint64_t *frames, uint64_t *drawn, int64_t n, const uint8_t *atlas_rgb, int ink_row0, int ink_row1,
                                  uint8_t *obs, int views, hipStream_t st) {
    if (n <= 0 || (views != 1 && views != 2)) return;
    const uint4 *at = reinterpret_cast<const uint4 *>(atlas_rgb);
    uint4 *ob = reinterpret_cast<uint4 *>(obs);
#define CRL_LAUNCH_DELTA(V, L, G)                                                                                                       \
    hipLaunchKernelGGL((pong_raster_raw_delta_kernel<V, L, G>), dim3((unsigned)((n * V * L + 255) / 256)), dim3(256), 0, st, frames, drawn, at, \
                       ink_row0, ink_row1, ob, n)
#ifdef CRL_ABLATION
    // (profiling build only: CRL_RAW_DELTA_L / CRL_RAW_DELTA_G select the lanes per (env, view) and the chunks per block that lost the
    // measurement, CRL_RAW_DELTA_LANES=1 the superseded lane-per-env mapping)
    static const int abl_lanes = getenv("CRL_RAW_DELTA_LANES") ? atoi(getenv("CRL_RAW_DELTA_LANES")) : 0;
    static const int abl_l = getenv("CRL_RAW_DELTA_L") ? atoi(getenv("CRL_RAW_DELTA_L")) : kDeltaL;
    static const int abl_g = getenv("CRL_RAW_DELTA_G") ? atoi(getenv("CRL_RAW_DELTA_G")) : kDeltaG;
    if (abl_lanes) {
        const unsigned blocks = (unsigned)((n + 63) / 64);
        if (views == 2)
            hipLaunchKernelGGL((pong_raster_raw_delta_lanes_kernel<2>), dim3(blocks), dim3(384), 0, st, frames, drawn, at, ink_row0, ink_row1, ob, n);
        else
            hipLaunchKernelGGL((pong_raster_raw_delta_lanes_kernel<1>), dim3(blocks), dim3(192), 0, st, frames, drawn, at, ink_row0, ink_row1, ob, n);
        return;
    }
    if (abl_l != kDeltaL || abl_g != kDeltaG) {
        const int g = (uintptr_t)obs % (16 * abl_g) ? 1 : abl_g;
#define CRL_DELTA_CASE(L, G)                \
    if (abl_l == L && g == G) {             \
        if (views == 2) CRL_LAUNCH_DELTA(2, L, G); \
        else CRL_LAUNCH_DELTA(1, L, G);     \
        return;                             \
    }
        CRL_DELTA_CASE(16, 1) CRL_DELTA_CASE(16, 2) CRL_DELTA_CASE(16, 4) CRL_DELTA_CASE(32, 1) CRL_DELTA_CASE(32, 2) CRL_DELTA_CASE(32, 4)
        CRL_DELTA_CASE(64, 1) CRL_DELTA_CASE(64, 2) CRL_DELTA_CASE(64, 4)
#undef CRL_DELTA_CASE
        return;  // (no such variant: nothing is drawn, which the tests see)
    }
#endif
    // a block is a whole sector only in a buffer aligned to it; crl_draw_raw_delta admits any 16-byte-aligned one: single chunks there
    const bool blocks_ok = (uintptr_t)obs % (16 * kDeltaG) == 0;
    if (views == 2) {
        if (blocks_ok) CRL_LAUNCH_DELTA(2, kDeltaL, kDeltaG);
        else CRL_LAUNCH_DELTA(2, kDeltaL, 1);
    } else {
        if (blocks_ok) CRL_LAUNCH_DELTA(1, kDeltaL, kDeltaG);
        else CRL_LAUNCH_DELTA(1, kDeltaL, 1);
    }
#undef CRL_LAUNCH_DELTA
}

void launch_pong_raster_raw(const uint64_t *frames, int64_t n, const uint8_t *atlas_rgb, int ink_row0, int ink_row1,
                            uint8_t *obs, int views, hipStream_t st) {
    if (n <= 0) return;
    // (profiling build only: CRL_RAW_DEBUG bit 1 = constant chunks, i.e. WRONG pixels, to size the pixel arithmetic; CRL_RAW_SWEEP /
    // CRL_RAW_LINEAR select the superseded writers)
    static const int dbg = CRL_ABL(getenv("CRL_RAW_DEBUG") ? atoi(getenv("CRL_RAW_DEBUG")) : 0);
    static const int sweep = CRL_ABL(getenv("CRL_RAW_SWEEP") != nullptr) ? atoi(getenv("CRL_RAW_SWEEP")) : 4;
    if (views != 1 && views != 2) return;  // (crl_create admits nothing else)
    if (sweep > 0) {
        const int64_t total = n * views * kFrameChunks;
        const uint4 *at = reinterpret_cast<const uint4 *>(atlas_rgb);
        uint4 *ob = reinterpret_cast<uint4 *>(obs);
#define CRL_LAUNCH_SWEEP(I, V)                                                                                              \
    hipLaunchKernelGGL((pong_raster_raw_sweep_kernel<I, V>), dim3((unsigned)((total + 256 * I - 1) / (256 * I))), dim3(256), 0, st, frames, \
                       at, ink_row0, ink_row1, ob, n, dbg)
        if (views == 2) {
#ifdef CRL_ABLATION
            if (sweep <= 2) CRL_LAUNCH_SWEEP(2, 2);
            else if (sweep > 4) CRL_LAUNCH_SWEEP(8, 2);
            else
#endif
                CRL_LAUNCH_SWEEP(4, 2);
        } else {
            CRL_LAUNCH_SWEEP(4, 1);
        }
#undef CRL_LAUNCH_SWEEP
        return;
    }
#ifdef CRL_ABLATION
    static const int lin = getenv("CRL_RAW_LINEAR") ? atoi(getenv("CRL_RAW_LINEAR")) : 2;
    if (lin > 0) {
        const int64_t total = n * views * kFrameChunks;
        const uint4 *at = reinterpret_cast<const uint4 *>(atlas_rgb);
        uint4 *ob = reinterpret_cast<uint4 *>(obs);
#define CRL_LAUNCH_LIN(I, V)                                                                                         \
    hipLaunchKernelGGL((pong_raster_raw_linear_kernel<I, 256, V>), dim3((unsigned)((total + 256 * I - 1) / (256 * I))), dim3(256), 0, \
                       st, frames, at, ink_row0, ink_row1, ob, views, n, dbg)
        if (views == 2) {
            if (lin <= 1) CRL_LAUNCH_LIN(1, 2);
            else if (lin <= 2) CRL_LAUNCH_LIN(2, 2);
            else if (lin <= 4) CRL_LAUNCH_LIN(4, 2);
            else CRL_LAUNCH_LIN(8, 2);
        } else {
            CRL_LAUNCH_LIN(2, 1);
        }
#undef CRL_LAUNCH_LIN
        return;
    }
    hipLaunchKernelGGL(pong_raster_raw_kernel, dim3((unsigned)n), dim3(256), 0, st, frames,
                       reinterpret_cast<const uint4 *>(atlas_rgb), ink_row0, ink_row1, reinterpret_cast<uint4 *>(obs), views, dbg);
#endif
}

}  // namespace crl

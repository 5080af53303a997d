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
// The work split is pong_raster_raw_sweep_kernel's: address-linear, a thread's four chunks a whole grid apart.
#include <stdlib.h>

#include "crl_internal.h"
#include "pong_band_span.h"
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
// the full draw and the delta draw below.
__device__ __forceinline__ uint4 raw_chunk(const Frame &f, int q, const uint4 *__restrict__ atlas_rgb, int ink_row0, int ink_row1) {
    const bool blank = f.sl == 255;
    const uint32_t bg = blank ? 0u : 0xFFFFFFFFu;
    const int view = q >= kFrameChunks;
    const int c = q - view * kFrameChunks;
    const int row = c / kRowChunks;
    const int cc = c - row * kRowChunks;
    const bool mirror = view && row >= CRL_PONG_MIRROR_ROW;
    const int sc = mirror ? (kRowChunks - 1 - cc) : cc;  // source chunk in the unmirrored row
    uint4 v = make_uint4(bg, bg, bg, bg);
    if (!blank) {
        if (row < CRL_PONG_TOP) {
            if (row >= ink_row0 && row < ink_row1) v = atlas_rgb[(int64_t)((f.sl * 22 + f.sr) * CRL_PONG_TOP + row) * kRowChunks + sc];
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

// Court rows only (TOP .. BOTTOM-1) of a frame that is not blank: the 16 bytes of source chunk sc of `row`, byte-reversed for the
// mirrored view.  What raw_chunk() stores there, without its division, its atlas pointer and its load: the delta writer's loops
// call this one, so that no store of theirs waits for a load.  The ball's 12 bytes are a shifted constant, each bat lies in one
// chunk column and enters as a constant mask, and since every pixel is achromatic the mirrored chunk is the chunk of the
// bit-reversed coverage mask.
static constexpr int kBallBytes = 3 * CRL_PONG_BALL, kBatBytes = 3 * CRL_PONG_BAT_W;
static constexpr int kBatLChunk = 3 * CRL_PONG_BATL_X / 16, kBatRChunk = 3 * CRL_PONG_BATR_X / 16;
static constexpr uint32_t kBatLMask = ((1u << kBatBytes) - 1u) << (3 * CRL_PONG_BATL_X - 16 * kBatLChunk);
static constexpr uint32_t kBatRMask = ((1u << kBatBytes) - 1u) << (3 * CRL_PONG_BATR_X - 16 * kBatRChunk);
static_assert(kBallBytes <= 16 && kBatLMask <= 0xFFFFu && kBatRMask <= 0xFFFFu, "a bat's bytes lie in one chunk; the ball's fit a chunk's mask");

__device__ __forceinline__ uint32_t nibble_to_bytes_perm(uint32_t nib) {
    // bit k of nib (< 16) -> byte k = 0xFF: a byte selector of 12 gives 0x00 and one of 13 gives 0xFF (no 32-bit multiply)
    return __builtin_amdgcn_perm(0u, 0u, (__umul24(nib, 0x00204081u) & 0x01010101u) | 0x0C0C0C0Cu);
}

__device__ __forceinline__ uint4 court_chunk(const Frame &f, int row, int sc, bool mirror) {
    // bits [a, a + 12) of the chunk's 16 are the ball's, a clamped to where the mask is empty: the shift stays within 0..28
    const int a = min(max(3 * f.x - 16 * sc, -kBallBytes), 16);
    uint32_t m = (unsigned)(row - f.y) < (unsigned)CRL_PONG_BALL ? ((((1u << kBallBytes) - 1u) << 16) >> (16 - a)) & 0xFFFFu : 0u;
    if (sc == kBatLChunk && (unsigned)(row - f.bl) < (unsigned)CRL_PONG_BAT_H) m |= kBatLMask;
    if (sc == kBatRChunk && (unsigned)(row - f.br) < (unsigned)CRL_PONG_BAT_H) m |= kBatRMask;
    if (mirror) m = __brev(m) >> 16;
    return make_uint4(nibble_to_bytes_perm(m & 15u), nibble_to_bytes_perm((m >> 4) & 15u), nibble_to_bytes_perm((m >> 8) & 15u),
                      nibble_to_bytes_perm(m >> 12));
}

// The full draw, address-linear (workgroups write chunks of the WHOLE output tensor, whichever envs they belong to: with one
// workgroup per env the ~2 000 resident workgroups write 2 000 separate streams 201 600 B apart, which DRAM sees as that many open
// pages): thread t of workgroup b writes chunks b * 256 + t + i * (gridDim.x * 256),
// i = 0 .. ITERS-1 -- every "round" i of the whole chip is one dense linear sweep over 1/ITERS of the tensor.  Pure-store
// probes (tools/store_order_probe.hip): a wavefront that walks through a private contiguous span makes the chip write a
// comb (one tooth per resident wavefront) and loses 8-20 % of the fill rate; stores a whole grid apart do not, however
// many a wavefront issues.  Per round a workgroup's 4 KB block touches at most two envs (two scalar descriptor loads).
template <int ITERS, int VIEWS>
__global__ __launch_bounds__(256) void pong_raster_raw_sweep_kernel(const uint64_t *__restrict__ frames, const uint4 *__restrict__ atlas_rgb,
                                                                    int ink_row0, int ink_row1, uint4 *__restrict__ obs, int64_t n) {
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
        obs[g] = raw_chunk(pick_frame(f0[i], f1[i], second), q, atlas_rgb, ink_row0, ink_row1);
    }
}

// Delta writer: the buffer an env draws into holds the frame of an earlier descriptor `drawn[env]` (the caller's record, see
// crl_draw_raw_delta), and a frame is a pure function of its descriptor, so only the chunks whose bytes can differ between the
// two descriptors are stored -- each still built by raw_chunk(), so the result is the full draw's, bit for bit.  Dirty set (a
// superset of the differing chunks for ANY pair of descriptors):
//   exactly one descriptor blank ..................... the whole frame;
//   both blank ....................................... nothing;
//   otherwise a single point (sl + 1 or sr + 1) ...... in the score-band ink rows [ink_row0, ink_row1), the chunk columns from the
//                                                      first to the last one in which the band images of the old and the new pair
//                                                      differ (pong_band_span.h: a table made from the atlas in crl_create; 2-3
//                                                      columns for most pairs of the shipped atlas, up to 12 where a number gains
//                                                      a digit), mirrored in the second view's rows >= CRL_PONG_MIRROR_ROW;
//            (sl, sr) differ in any other way ........ every chunk of the ink rows (a game's end, set_state, scores outside the atlas);
//            and in rows TOP..BOTTOM-1, per object:   ball: the chunks of both 4 x 4 rectangles;
//                                                     bat:  its chunk column in the rows of the symmetric difference of its old
//                                                           and new 15-row spans (<= 8 rows for a 4-px move).
// A pixel of the court is white iff the ball or a bat covers it, so a pixel that changes lies in the symmetric difference of
// some object's two rectangles; rows outside the court and the ink rows are white in every non-blank frame.
// Mapping: a group of 32 lanes owns one (env, view), so the stores of one instruction go side by side into one frame instead of
// into 64 frames 201 600 B apart, and walks the objects one after another: the new ball, the old ball, the left bat, the right bat.
// Within an object a lane's place is fixed by its lane id alone -- the chunk of the block fastest (G = 4 adjacent lanes: a whole
// aligned 64-byte memory request), then for a ball the block of the row (its 12 bytes touch at most two), then the row -- and the
// lane only tests whether that place is dirty: row inside the court, block no further than the rectangle's last.  A ball is one
// store instruction, a bat one per eight rows of the symmetric difference of its two spans (its single chunk column makes one
// block a row).  With two views the descriptors are wave-uniform, so the rectangles, the trip counts and every branch are scalar
// code, and the mirrored view differs by o -> 29 - o per lane.  Blocks are counted from the buffer's start: a row starts 0 or 2
// chunks into a block, so a ball's block can reach two chunks into the neighbouring row, which is a court row too.  Every chunk
// stored is built from the NEW descriptor by court_chunk(): the chunks of a block that are not dirty are rewritten with the bytes
// they hold.  Blocks of the old ball's rectangle that the new one covers are stored once.  Two lanes may still store the same
// block (the ball over a bat's column): both write the new frame's bytes, so the race is benign.  A point's span is laid out the
// same way -- chunk of the block, block of the row (per lane `blk <= the row's last block`: a row starts 0 or 2 chunks into a block),
// ink row -- with every chunk, a block's clean ones and those it holds of the neighbouring row included, built from the new descriptor
// by raw_chunk() from its absolute index.  Whole frames and whole score bands are strided over by the same lanes through raw_chunk().
// The record is read and then written by the env's own wavefront.  A buffer that is not 64-byte aligned takes G = 1: single chunks,
// exactly the dirty set.
// After a synchronous reset the envs score in step with one another: a launch in which 80-94 % of the envs redraw a band (every
// ~20th step and the one after it: each of the two buffers sees the point once) is what the spread between launches consists of.
// Measured on MI355X at 65 536 envs, two views, the launch inside the bench's event brackets (profiles/r08_raw_summary.txt):
//   one lane per env, 16-byte chunks (round 7) ........ 164 us   3.5 M memory write requests, 95 % of them 32-byte with a mask
//   L = 32, G = 1 / G = 2 (whole 32-byte sectors) ..... 168 / 164 us   (the requests neither merge nor get cheaper)
//   L = 32, G = 4 (whole 64-byte blocks) ..............  97 us   (88.6 against the round-7 mapping's 151 on a second box)
//   L = 16 / 64, G = 4 ................................ 101 / 108 us on that second box
// The cost was the partial memory request, not the byte count (G = 4 writes 198 MB against 118.7) and not the lane order.
// Round 9 (profiles/r09_raw_summary.txt): the mapping above against the one before it (running sums over six rectangles, slot ->
// rectangle decoded per trip, chunks built by raw_chunk()), alternating runs on one box:
//   vector / scalar instructions per wavefront ........ 516 / 295 -> 272 / 148 (SQ counters); no load and no vmcnt wait in the court code
//   the launch inside the bench's event brackets ....... 96.4 -> 91.3 us; the step 0.1103 -> 0.1051 ms; same requests, same bytes
// Half the instructions bought a twentieth of the time: the launch is bound by its 3.1 M scattered 64-byte requests, not by issue.
// Round 10 (profiles/r10_raw_summary.txt): a launch in which 94 % of the envs redraw the whole band holds 20.9 M requests against a
// court-only launch's 3.1 M and takes 6 x as long; with a point's span it holds 8.7 M (48 per env for the band, the rest because the
// serve after a point moves the ball and both bats in the same step).  Alternating runs on one box:
//   the launch inside the bench's event brackets ....... 91.4 -> 66.6 us; the step 0.1052 -> 0.0803 ms; the longest launch 436 -> 171 us
static constexpr int kDeltaL = 32, kDeltaG = 4;  // lanes per (env, view); chunks per block (4: whole 64-byte memory requests)
static_assert(kFrameChunks % kDeltaG == 0, "a view starts on a block boundary");
// The one-launch step: the envs of a workgroup (kStepB) and of one of its wavefronts (kStepW; one view: two, a trip's worth).  Whether the
// stores carry the non-temporal hint: the draw-only kernel's do not (kDeltaNT), the one-launch step's do (kStepNT) -- its workgroups
// read and write the env state while others store pixels.  All chosen by measurement (profiles/r11_raw_summary.txt).
static constexpr int kStepW = 1, kStepB = 16;
static constexpr bool kDeltaNT = false, kStepNT = true;

// a 16-byte store of the delta writer; NT: with the non-temporal hint (the same bytes either way)
typedef uint32_t crl_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ void chunk_store(uint4 *p, const uint4 &v) {
    if (NT) __builtin_nontemporal_store(crl_u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<crl_u32x4 *>(p));
    else *p = v;
}

// one court chunk of the view: q counts the view's chunks, q_row is the first chunk of `row`.  WRAP: q may lie up to two chunks
// into the row above or below (a ball's block); a bat's block never leaves its row.
template <bool WRAP, bool NT>
__device__ __forceinline__ void court_store(uint4 *__restrict__ out, int q_view, const Frame &f, bool mirror, int row, int q_row, int q) {
    int o = q - q_row;
    if (WRAP) {
        const int w = (o >= kRowChunks) - (o < 0);
        row += w, o -= w * kRowChunks;
    }
    chunk_store<NT>(reinterpret_cast<uint4 *>(reinterpret_cast<char *>(out) + (uint32_t)((q_view + q) * 16)), court_chunk(f, row, mirror ? kRowChunks - 1 - o : o, mirror));
}

// the source chunks [c0, c1] a ball at x covers; ok: some byte of it lies inside the row
struct BallCols {
    int c0, c1;
    bool ok;
};
__device__ __forceinline__ BallCols ball_cols(int x) {
    const int b0 = max(3 * x, 0), b1 = min(3 * x + kBallBytes, kRowBytes);
    BallCols c;
    c.ok = b0 < b1, c.c0 = b0 >> 4, c.c1 = (max(b1, 1) - 1) >> 4;
    return c;
}

// The delta draw of one (env, view) by its group of kDeltaL lanes: everything above from the blank tests on.  pn / po: the new
// descriptor and the one the buffer holds; out: the env's first chunk.  Shared by the draw-only kernel and the one-launch step
// below.  NT: the stores carry the non-temporal hint (profiles/r11_raw_summary.txt).
template <int G, bool NT>
__device__ __forceinline__ void raw_delta_draw(uint64_t pn, uint64_t po, int view, int lane, uint4 *__restrict__ out, const uint4 *__restrict__ atlas_rgb,
                                               const uint8_t *__restrict__ band_span, int ink_row0, int ink_row1) {
    static_assert(G == 1 || G == 4, "");
    constexpr int L = kDeltaL, SH = G == 4 ? 2 : 0;
    const Frame f = unpack_frame(pn), g = unpack_frame(po);
    const bool blank_n = f.sl == 255, blank_o = g.sl == 255;
    if (blank_n && blank_o) return;  // (two blank frames are equal)
    const int q_view = view * kFrameChunks;
    if (blank_n != blank_o) {  // the whole frame
        for (int c = lane; c < kFrameChunks; c += L) chunk_store<NT>(out + (q_view + c), raw_chunk(f, q_view + c, atlas_rgb, ink_row0, ink_row1));
        return;
    }
    const int j = lane & (G - 1), u = lane >> SH;  // this lane's chunk of a block; its (row, block) place within an object
    if ((f.sl != g.sl || f.sr != g.sr) && ink_row1 > ink_row0) {  // the score band's ink rows
        // a single point: the source chunk columns [s0, s1] in which the two band images differ, from the table of the old pair
        const int kind = f.sl == g.sl;  // 0: left + 1, 1: right + 1
        int s0 = kBandWholeFirst, s1 = kBandWholeLast;
        if (band_span && g.sl < 22 && g.sr < 22 && f.sl == g.sl + 1 - kind && f.sr == g.sr + kind) {
            // (a pair's two entries are one dword: a scalar load where the descriptors are wave-uniform)
            const uint32_t e = reinterpret_cast<const uint32_t *>(band_span)[g.sl * 22 + g.sr] >> (16 * kind);
            s0 = e & 255, s1 = (e >> 8) & 255;
        }
        if (s1 >= kRowChunks) {  // every other pair (a game's end, set_state, a successor outside the atlas): every chunk of the ink rows
            const int c0 = q_view + ink_row0 * kRowChunks, cn = (ink_row1 - ink_row0) * kRowChunks;
            for (int c = lane; c < cn; c += L) chunk_store<NT>(out + (c0 + c), raw_chunk(f, c0 + c, atlas_rgb, ink_row0, ink_row1));
        } else if (s0 <= s1) {
            // place = (ink row, block of the row): a row's span touches at most nb blocks (it starts anywhere within its first
            // block), 1 << bs >= nb of them are a row's share of a trip's L / G places, and a trip takes (L / G) >> bs rows
            const int w = s1 - s0 + 1, nb = G == 1 ? w : (w + 2 * G - 2) >> SH;
            int bs = 0;
            while ((1 << bs) < nb && (1 << bs) < (L >> SH)) bs++;
            const int dr = u >> bs, bu = u & ((1 << bs) - 1);
            for (int r0 = ink_row0; r0 < ink_row1; r0 += (L >> SH) >> bs) {
                const int row = r0 + dr, q_row = q_view + row * kRowChunks;
                const bool mir = view != 0 && row >= CRL_PONG_MIRROR_ROW;
                const int first = (q_row + (mir ? kRowChunks - 1 - s1 : s0)) >> SH, last = (q_row + (mir ? kRowChunks - 1 - s0 : s1)) >> SH;
                for (int b0 = 0; b0 < nb; b0 += 1 << bs) {
                    const int blk = first + b0 + bu, q = (blk << SH) + j;  // (a block may reach into the neighbouring row: raw_chunk() draws that row's chunk)
                    if (row < ink_row1 && blk <= last) chunk_store<NT>(out + q, raw_chunk(f, q, atlas_rgb, ink_row0, ink_row1));
                }
            }
        }
    }

    const bool mirror = view != 0;  // (court rows are all >= CRL_PONG_MIRROR_ROW)
    auto in_court = [](int row) { return (unsigned)(row - CRL_PONG_TOP) < (unsigned)(CRL_PONG_BOTTOM - CRL_PONG_TOP); };

    if (f.x != g.x || f.y != g.y) {  // the two balls: place u = (row of the ball, first or second block of the row)
        const BallCols cn = ball_cols(f.x), co = ball_cols(g.x);
        const int n0 = mirror ? kRowChunks - 1 - cn.c1 : cn.c0, n1 = mirror ? kRowChunks - 1 - cn.c0 : cn.c1;
        const int o0 = mirror ? kRowChunks - 1 - co.c1 : co.c0, o1 = mirror ? kRowChunks - 1 - co.c0 : co.c1;
        const int dr = u >> 1, b = u & 1;
        if (cn.ok) {
            const int row = f.y + dr, q_row = row * kRowChunks, blk = ((q_row + n0) >> SH) + b;
            if (dr < CRL_PONG_BALL && in_court(row) && blk <= ((q_row + n1) >> SH)) court_store<true, NT>(out, q_view, f, mirror, row, q_row, (blk << SH) + j);
        }
        if (co.ok) {
            const int row = g.y + dr, q_row = row * kRowChunks, blk = ((q_row + o0) >> SH) + b;
            const bool again = cn.ok && (unsigned)(row - f.y) < (unsigned)CRL_PONG_BALL && blk >= ((q_row + n0) >> SH) && blk <= ((q_row + n1) >> SH);
            if (dr < CRL_PONG_BALL && in_court(row) && blk <= ((q_row + o1) >> SH) && !again)  // (again: the new ball's rectangle stores this block)
                court_store<true, NT>(out, q_view, f, mirror, row, q_row, (blk << SH) + j);
        }
    }
    // a bat: the rows of the symmetric difference of [a, a + h) and [b, b + h) are [lo, lo + k) and [hi + h - k, hi + h),
    // k = min(|a - b|, h); place t = one of these 2k rows, its one block
    auto bat = [&](int a, int b, int sc) {
        const int lo = min(a, b), hi = max(a, b), k = min(hi - lo, CRL_PONG_BAT_H), up = hi + CRL_PONG_BAT_H - 2 * k;
        const int o = mirror ? kRowChunks - 1 - sc : sc;
        int lo_q = lo * kRowChunks, up_q = up * kRowChunks, u_q = u * kRowChunks;  // row * 30 as a sum of products made once ...
        asm("" : "+v"(u_q));  // ... which the compiler folds back into a quarter-rate 32-bit multiply per trip unless one term is opaque
        for (int t0 = 0; t0 < 2 * k; t0 += L >> SH) {
            const int t = t0 + u, row = (t < k ? lo : up) + t, q_row = (t < k ? lo_q : up_q) + t0 * kRowChunks + u_q;
            if (t < 2 * k && in_court(row)) court_store<false, NT>(out, q_view, f, mirror, row, q_row, ((q_row + o) & ~(G - 1)) + j);
        }
    };
    bat(g.bl, f.bl, kBatLChunk);
    bat(g.br, f.br, kBatRChunk);
}

template <int VIEWS, int G, bool NT>
__global__ __launch_bounds__(256) void pong_raster_raw_delta_kernel(const uint64_t *__restrict__ frames, uint64_t *__restrict__ drawn,
                                                                    const uint4 *__restrict__ atlas_rgb, const uint8_t *__restrict__ band_span,
                                                                    int ink_row0, int ink_row1, uint4 *__restrict__ obs, int64_t n) {
    static_assert(VIEWS == 1 || VIEWS == 2, "");
    constexpr int L = kDeltaL, per_env = VIEWS * kFrameChunks;
    constexpr int E = 64 / L / VIEWS;  // whole envs per wavefront: one with two views -> uniform descriptor loads
    const int64_t gw = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);  // this wavefront, of the grid
    const int lane = (int)threadIdx.x & (L - 1), sub = ((int)threadIdx.x & 63) / L;
    const int64_t env = gw * E + (E > 1 ? sub / VIEWS : 0);
    const int view = sub % VIEWS;
    const bool valid = env < n;
    const uint64_t pn = valid ? frames[env] : kBlankFrame, po = valid ? drawn[env] : kBlankFrame;
    if (valid && view == 0 && lane == 0) drawn[env] = pn;
    if (!valid) return;
    raw_delta_draw<G, NT>(pn, po, view, lane, obs + env * per_env, atlas_rgb, band_span, ink_row0, ink_row1);
}

// A raw step in one launch: raw_step_env() and the delta draw above in the same workgroup, so the step has no second launch, no
// kernel boundary in front of the draw and no descriptor round trip through obs_frames[].  A workgroup owns B consecutive envs
// and is B / W wavefronts.  Phase A: lanes 0 .. B-1 of its first wavefront step one env each (SoA state: coalesced loads and
// stores), swap the new descriptors into the record and hand old and new to the others through LDS behind one barrier; the
// others wait there and issue nothing.  Phase B: wavefront w holds the descriptors of envs w * W .. w * W + W - 1 in its lanes
// 0 .. W-1 (every other lane: two blank ones, which the draw skips) and walks them, 64 / kDeltaL / VIEWS per trip as the draw-only
// kernel's wavefronts do, taking each env's pair out of its lane -- with two views by readlane at the uniform trip index, so the
// rectangles, trip counts and branches of raw_delta_draw() stay scalar code; with one view each 32-lane group fetches its env's
// pair by a shuffle.  stepped: phase A only reads the descriptors a dynamics launch left; always 0 (kept: without the argument the
// unaligned two-view instance allocates two scalar registers more).
// Measured on MI355X at 65 536 envs, two views, variants alternated inside one process over bench.py's window (r11_raw_summary.txt):
//   draw-only kernel behind the dynamics kernel ....... 68.6 + 5.4 us in their brackets, the step 0.0825 ms
//   first design: no LDS, every wavefront steps its own W = 16 envs in 16 lanes and draws them in sequence ... 78.0 us, 0.0826 ms
//   B = 64, W = 8 / 16 / 32 / 64, plain stores ........ 81.5 / 77.2 / 82.1 / 91.8 us; phase B of W = 16 alone 73.9 us: envs in sequence
//                                                       in one wavefront cost 7 us against one short wavefront per env, phase A 2 us
//   B = 16, W = 1 (the draw-only kernel's mapping) .... 96.2 us with plain stores, 75.2 us with non-temporal ones, the step 0.0794 ms
//   W = 1 B = 4 / 8, W = 2 B = 16 / 32, W = 4 B = 32 / 64, W = 8 / 16 B = 64, non-temporal ... 75.6-77.1 us
// Workgroups outnumber the chip's slots at B = 16, so later ones step while earlier ones store; their state loads then compete
// with pixel lines in the L2s unless the pixels bypass them.  The draw-only kernel is 1.7 us slower with the hint and keeps plain stores.
template <int VIEWS, int G, int W, int B, bool NT>
__global__ __launch_bounds__(64 * (B / W)) void pong_step_raw_delta_kernel(
    PongSoA s, ServeSrc src, const int32_t *__restrict__ actions, int64_t n, float *__restrict__ rew, uint8_t *__restrict__ done_out,
    uint64_t *__restrict__ drawn, const uint4 *__restrict__ atlas_rgb, const uint8_t *__restrict__ band_span, int ink_row0, int ink_row1,
    uint4 *__restrict__ obs, int stepped) {
    constexpr int L = kDeltaL, per_env = VIEWS * kFrameChunks;
    constexpr int E = 64 / L / VIEWS;  // envs per trip of phase B
    static_assert((VIEWS == 1 || VIEWS == 2) && B <= 64 && B % W == 0 && B / W <= 16 && W % E == 0 && (W & (W - 1)) == 0, "");
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), wl = (int)threadIdx.x & 63;
    const int64_t b0 = (int64_t)blockIdx.x * B, e0 = b0 + wave * W;  // the workgroup's first env, this wavefront's
    __shared__ uint64_t hand[2][B];
    if (wave == 0 && wl < B) {
        uint64_t pn = kBlankFrame, po = kBlankFrame;
        const int64_t i = b0 + wl;
        if (i < n) {
            po = drawn[i];
            pn = stepped ? s.obs_frames[i] : raw_step_env(s, src, actions, i, n, rew, done_out, VIEWS == 1);
            drawn[i] = pn;
        }
        hand[0][wl] = pn, hand[1][wl] = po;
    }
    __syncthreads();
    const int k = wave * W + (wl & (W - 1));
    const uint64_t pn = wl < W ? hand[0][k] : kBlankFrame, po = wl < W ? hand[1][k] : kBlankFrame;
    const int lane = wl & (L - 1), sub = wl / L;
#pragma unroll 1
    for (int t = 0; t < W; t += E) {
        if (e0 + t >= n) break;  // (uniform)
        uint32_t nl, nh, ol, oh;
        if (VIEWS == 2) {
            nl = __builtin_amdgcn_readlane((uint32_t)pn, t), nh = __builtin_amdgcn_readlane((uint32_t)(pn >> 32), t);
            ol = __builtin_amdgcn_readlane((uint32_t)po, t), oh = __builtin_amdgcn_readlane((uint32_t)(po >> 32), t);
        } else {
            nl = __shfl((uint32_t)pn, t + sub), nh = __shfl((uint32_t)(pn >> 32), t + sub);
            ol = __shfl((uint32_t)po, t + sub), oh = __shfl((uint32_t)(po >> 32), t + sub);
        }
        // (an env past n holds two blank descriptors: nothing is stored through its pointer)
        const int64_t env = e0 + t + (VIEWS == 1 ? sub : 0);
        raw_delta_draw<G, NT>(((uint64_t)nh << 32) | nl, ((uint64_t)oh << 32) | ol, VIEWS == 2 ? sub : 0, lane, obs + env * per_env, atlas_rgb, band_span,
                              ink_row0, ink_row1);
    }
}

void launch_pong_raster_raw_delta(const uint64_t *frames, uint64_t *drawn, int64_t n, const uint8_t *atlas_rgb, const uint8_t *band_span,
                                  int ink_row0, int ink_row1, uint8_t *obs, int views, hipStream_t st) {
    if (n <= 0 || (views != 1 && views != 2)) return;
    const uint4 *at = reinterpret_cast<const uint4 *>(atlas_rgb);
    uint4 *ob = reinterpret_cast<uint4 *>(obs);
    // a block is a whole memory request only in a buffer aligned to it; crl_draw_raw_delta admits any 16-byte-aligned one: single chunks there
    const bool blocks_ok = (uintptr_t)obs % (16 * kDeltaG) == 0;
#define CRL_LAUNCH_DELTA_SPAN(V, G, NT)                                                                                                    \
    hipLaunchKernelGGL((pong_raster_raw_delta_kernel<V, G, NT>), dim3((unsigned)((n * V * kDeltaL + 255) / 256)), dim3(256), 0, st, frames, drawn, at, \
                       band_span, ink_row0, ink_row1, ob, n)
    if (views == 2) {
        if (blocks_ok) CRL_LAUNCH_DELTA_SPAN(2, kDeltaG, kDeltaNT);
        else CRL_LAUNCH_DELTA_SPAN(2, 1, kDeltaNT);
    } else {
        if (blocks_ok) CRL_LAUNCH_DELTA_SPAN(1, kDeltaG, kDeltaNT);
        else CRL_LAUNCH_DELTA_SPAN(1, 1, kDeltaNT);
    }
#undef CRL_LAUNCH_DELTA_SPAN
}

void launch_pong_step_raw_delta(const PongSoA &s, const ServeSrc &src, const int32_t *actions, int64_t n, float *rew, uint8_t *done,
                                uint64_t *drawn, const uint8_t *atlas_rgb, const uint8_t *band_span, int ink_row0, int ink_row1, uint8_t *obs,
                                int views, hipStream_t st) {
    if (n <= 0 || (views != 1 && views != 2)) return;
    const uint4 *at = reinterpret_cast<const uint4 *>(atlas_rgb);
    uint4 *ob = reinterpret_cast<uint4 *>(obs);
    const bool blocks_ok = (uintptr_t)obs % (16 * kDeltaG) == 0;  // (as in launch_pong_raster_raw_delta)
#define CRL_LAUNCH_STEP(V, G, W, B, NT)                                                                                                          \
    hipLaunchKernelGGL((pong_step_raw_delta_kernel<V, G, W, B, NT>), dim3((unsigned)((n + B - 1) / B)), dim3(64 * (B / W)), 0, st, s, src, actions, n, rew, \
                       done, drawn, at, band_span, ink_row0, ink_row1, ob, 0)
    constexpr int W1 = kStepW < 2 ? 2 : kStepW;  // (one view: a trip takes two envs)
    if (views == 2) {
        if (blocks_ok) CRL_LAUNCH_STEP(2, kDeltaG, kStepW, kStepB, kStepNT);
        else CRL_LAUNCH_STEP(2, 1, kStepW, kStepB, kStepNT);
    } else {
        if (blocks_ok) CRL_LAUNCH_STEP(1, kDeltaG, W1, kStepB, kStepNT);
        else CRL_LAUNCH_STEP(1, 1, W1, kStepB, kStepNT);
    }
#undef CRL_LAUNCH_STEP
}

void launch_pong_raster_raw(const uint64_t *frames, int64_t n, const uint8_t *atlas_rgb, int ink_row0, int ink_row1,
                            uint8_t *obs, int views, hipStream_t st) {
    if (n <= 0 || (views != 1 && views != 2)) return;  // (crl_create admits nothing else)
    const int64_t total = n * views * kFrameChunks;
    const uint4 *at = reinterpret_cast<const uint4 *>(atlas_rgb);
    uint4 *ob = reinterpret_cast<uint4 *>(obs);
    const unsigned blocks = (unsigned)((total + 256 * 4 - 1) / (256 * 4));
    if (views == 2) hipLaunchKernelGGL((pong_raster_raw_sweep_kernel<4, 2>), dim3(blocks), dim3(256), 0, st, frames, at, ink_row0, ink_row1, ob, n);
    else hipLaunchKernelGGL((pong_raster_raw_sweep_kernel<4, 1>), dim3(blocks), dim3(256), 0, st, frames, at, ink_row0, ink_row1, ob, n);
}

}  // namespace crl

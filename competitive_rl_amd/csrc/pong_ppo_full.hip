// pong_ppo_full.hip -- the learner's PPO update for the full-size ActorCritic on the device (include/crl.h "ppo update, full size"): the
// gradient of the clipped-surrogate loss over a minibatch of a crl_rollout, read from the stored uint8 planes, on a master blob in the
// layout of a full-size crl_policy (pong_policy_full.h).  The sample fetch, the loss and the statistics are pong_ppo.h's; the blobs'
// host side and the optimiser step are pong_ppo.hip's, over 1 001 784 floats; the reduce kernel is pong_ppo.h's.
//
// A minibatch is cut into chunks of at most scratch_rows samples (scratch per row: act2 / dz2 3872 floats, a3 256, dz3 256, dlogits and
// dv 4, the statistics 5 doubles); the chunks run in order, eight launches each, and every gradient element accumulates over the chunks
// in chunk order:
//   front     a sample per workgroup pass: the stack from the planes by the stack rule (a masked plane as zeros), conv1 + ReLU into LDS
//             inside conv2's zero border, conv2 + ReLU out to act2 -- policy_full_front_kernel's arithmetic (conv1 on
//             v_mfma_f32_16x16x32_bf16 with exact operands, conv2 on v_mfma_f32_16x16x4_f32) without its ring and its prefetch;
//   conv3     a3 = relu(act2 x W3^T + b3): policy_full_conv3_kernel's 128 x 128 x 16 LDS tiles, but K in 11 segments of 352 that each
//             start from zero and are added up in order.  The served kernel runs all 3872 products of a feature through one float32
//             accumulator (v_mfma_f32_16x16x4_f32 rounds after every product); that left a sample's log-probability up to 1.5e-6
//             off float64 and the approximate KL of a batch of 8 outside its budget (docs/LAB_NOTES_ppo_full_update.md);
//   heads     a wavefront per sample: logits and v in float64 (lane l: features l, l + 64, l + 128, l + 192, then a butterfly), the closed
//             forms of pong_ppo.h, dlogits / dv rounded once to float32, dz3 = (Wa^T dlogits + wc dv) * (a3 > 0);
//   head grad a thread per element of wa, wc, b3, ba, bc and per statistic: sums over slices of 256 rows, then the slices in order;
//   gW3       dz3^T x act2 (M 256, N 3872, K = rows): a workgroup owns a 128 x 32 tile of the output, a wavefront 32 x 32 of it in four
//             accumulators that START from the previous chunks' sum, and walks the rows four at a time in order; both operands are
//             contiguous along M / N, so each k-row is read coalesced straight from global memory;
//   dz2       (dz3 x W3) * (act2 > 0) (M = rows, N 3872, K 256), written over act2 by the thread that read it; K dealt kq-major as in
//             pong_policy_full.hip (lane kq of the instruction's four k lanes takes k = 16 g + 4 kq + j in step j: one 16-byte read of dz3);
//   back      workgroup w of W takes the chunk's rows w, w + W, ...: conv1 again into LDS, the row's dz2 into LDS, then
//               gW2[oc][ic, tap] += dz2[oc][pos] a1pad[ic][pos + tap]     M 32, N 256, K = 121 positions (4 per step, 3 zero ones at the end)
//               da1 in gather form, per parity class (py, px) of the padded a1 position (2 yh + py, 2 xh + px), yh, xh in 1 .. 10:
//                 da1[ic][pos] = sum over oc, a, b in {0, 1} of W2[oc][ic][py + 2 a][px + 2 b] dz2[oc][yh - a][xh - b]   (K = 32 x 4)
//               dz1 = da1 * (a1 > 0) into LDS, then gW1[oc][ic, tap] += dz1[oc][pos] x[ic][pos + tap]   M 16, N 64, K = 400
//             with gW1 / gW2 in matrix accumulators for the whole launch and the biases as per-thread sums beside them; the workgroup's
//             partial blob (9 264 floats: w1 | b1 | w2 | b2) is written by the first chunk and added to by the later ones.
// Then pong_ppo.h's reduce (the back kernel's partials in workgroup order for w1 .. b2, the accumulated sums for the rest, / float32(B),
// sums of squares per block of 256) and final (the block sums, the statistics).
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "crl_internal.h"
#include "pong_net.h"
#include "pong_policy_full.h"
#include "pong_ppo.h"
#include "pong_ring.h"
#include "pong_rollout.h"

namespace crl {

static constexpr int kBackBlob = kOffW3;      // 9 264: what the back kernel's partials hold (w1 | b1 | w2 | b2 of pong_policy_full.h's blob)
static constexpr int kBackMax = 256;          // W <= 256
static constexpr int kSqBlocks = (kFullBlob + 255) / 256;  // 3 914
static constexpr int64_t kDefaultRows = 16384;            // scratch: 17.6 KB per row = 288 MB
static constexpr int64_t kMinRows = 64, kMaxRows = 1 << 20;  // (eight launches per chunk: a smaller chunk only queues launches)

static constexpr int kS1Rows = 24, kS1Pitch = 580;  // a1: padded plane 24 x 24 = 576 floats + 4 (pong_policy_full.hip)
static constexpr int kW2Pitch = 260;                // W2 in LDS, floats per output channel
static constexpr int kDz2Pitch = 125;               // dz2 in LDS: 121 positions + 3 zeros, odd pitch
static constexpr int kDz1Pitch = 401;               // dz1 in LDS: 400 positions, odd pitch
static constexpr int kBackLdsFloats = kC2 * kW2Pitch + kC1 * kS1Pitch + kC2 * kDz2Pitch + kC1 * kDz1Pitch;
static constexpr int kBackLds = kBackLdsFloats * 4 + CRL_POLICY_STACK * kPlanePad;  // 119 168 bytes
static_assert(kBackLds <= 160 * 1024, "the back kernel's LDS must fit a CU");

struct PpoFull {
    int64_t scratch_rows = 0;
    int cus = 256;
    float *act2 = nullptr;   // [rows][3872]: a2, then dz2
    float *a3 = nullptr;     // [rows][256]
    float *dz3 = nullptr;    // [rows][256]
    float *dh = nullptr;     // [rows][4]: dlogits, dv
    double *st = nullptr;    // [rows][kStatN] (a teacher gradient: [rows][kStatAll]; so hsd and stat_acc)
    float *gacc = nullptr;   // [kFullBlob]: the sums over the samples of w3, b3, wa, ba, wc, bc (the rest and the pads stay zero)
    float *partials = nullptr;  // [kBackMax][kBackBlob]
    float *hs = nullptr;     // [ceil(rows / 256)][6 * 256]: the head gradients' slice sums
    double *hsd = nullptr;   // [ceil(rows / 256)][kStatN]: the statistics' slice sums
    double *stat_acc = nullptr, *sq_part = nullptr;
};

#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// conv1's B operands of a lane: channel li, k order 32 h + 8 lk + j = torch's own, each weight / 255 as three bf16 terms
__device__ __forceinline__ void conv1_weights(const float *__restrict__ w1, int li, int lk, bf8 (&wB)[3][2]) {
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            __bf16 t0, t1, t2;
            split_bf16x3(w1[li * 64 + 32 * h + 8 * lk + j] / 255.0f, t0, t1, t2);
            wB[0][h][j] = t0, wB[1][h][j] = t1, wB[2][h][j] = t2;
        }
}

// conv1 + ReLU of sample `flat` into the padded planes s1 (whose border is zero and stays so): the wavefront's tiles wave, wave + 4, ...
// of 25, as policy_full_front_kernel forms them; the spare turns repeat tile 24 (same values, same addresses).
__device__ __forceinline__ void conv1_to_lds(const RolloutView &r, uint32_t flat, const bf8 (&wB)[3][2], const f4 bias1, float *s1, int wave, int li,
                                             int lk) {
    const SampleAt at = sample_at(r, flat);
    const int depth = r.depth[flat];
    const uint8_t *pl[2];
    bool live[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {  // plane 2 h + (lk >> 1), window rows 2 (lk & 1) + {0, 1}
        const int j = 2 * h + (lk >> 1);
        live[h] = CRL_POLICY_STACK - 1 - j < depth;
        pl[h] = reinterpret_cast<const uint8_t *>(plane_of(r, at, j)) + (2 * (lk & 1)) * kDim;
    }
#pragma unroll
    for (int it = 0; it < 7; it++) {
        const int tl = min(wave + 4 * it, kP1 / 16 - 1);
        const int p = tl * 16 + li, y = p / 20, x = p - y * 20, off = 2 * y * kDim + 2 * x;
        bf8 ax[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t a = 0u, c = 0u;
            if (live[h]) {
                __builtin_memcpy(&a, pl[h] + off, 4);
                __builtin_memcpy(&c, pl[h] + off + kDim, 4);
            }
            const u32x4 v = {pk_bytes_bf16(a), pk_bytes_bf16(a >> 16), pk_bytes_bf16(c), pk_bytes_bf16(c >> 16)};
            ax[h] = __builtin_bit_cast(bf8, v);
        }
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tm = 2; tm >= 0; tm--)  // smallest weight term first
#pragma unroll
            for (int h = 0; h < 2; h++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wB[tm][h], ax[h], acc, 0, 0, 0);
        float *o = s1 + 4 * lk * kS1Pitch + (y + 2) * kS1Rows + x + 2;  // D: channels 4 lk + r x position li
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) o[r4 * kS1Pitch] = fmaxf(acc[r4] + bias1[r4], 0.f);
    }
}

// ---- front: act2[row] = relu(conv2(relu(conv1(stack / 255))))
__global__ __launch_bounds__(256) void ppo_full_front_kernel(RolloutView r, const int64_t *__restrict__ idx, int64_t rows, const float *__restrict__ raw,
                                                             float *__restrict__ act2) {
    __shared__ __attribute__((aligned(16))) float sw[kC2 * kW2Pitch];
    __shared__ __attribute__((aligned(16))) float s1[kC1 * kS1Pitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const float *w2 = raw + kOffW2, *b1 = raw + kOffB1, *b2 = raw + kOffB2;
    for (int i = tid; i < kC2 * 64; i += 256) {
        const int rr = i >> 6, c = i & 63;
        *reinterpret_cast<f4 *>(sw + rr * kW2Pitch + 4 * c) = *reinterpret_cast<const f4 *>(w2 + rr * 256 + 4 * c);
    }
    for (int i = tid; i < kC1 * kS1Pitch; i += 256) s1[i] = 0.f;  // the border stays zero
    bf8 wB[3][2];
    conv1_weights(raw + kOffW1, li, lk, wB);
    f4 bias1, bias2[2];  // D rows = channels 4 lk + r
#pragma unroll
    for (int q = 0; q < 4; q++) bias1[q] = b1[4 * lk + q], bias2[0][q] = b2[4 * lk + q], bias2[1][q] = b2[16 + 4 * lk + q];
    const float *swa = sw + li * kW2Pitch + 4 * lk, *swb = swa + 16 * kW2Pitch;
    int ao[2];  // conv2: the window row lk of position 32 wave + 16 u + li in the padded plane
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int pos = min(32 * wave + 16 * u + li, kP2 - 1), y = pos / 11, x = pos - 11 * y;
        ao[u] = (2 * y + lk) * kS1Rows + 2 * x;
    }
    __syncthreads();
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        conv1_to_lds(r, sample_of(r, idx, row), wB, bias1, s1, wave, li, lk);
        __syncthreads();
        f4 acc[2][2];
#pragma unroll
        for (int u = 0; u < 2; u++) acc[u][0] = f4{0.f, 0.f, 0.f, 0.f}, acc[u][1] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int g = 0; g < kC1; g++) {
            const f4 wa = *reinterpret_cast<const f4 *>(swa + 16 * g), wb = *reinterpret_cast<const f4 *>(swb + 16 * g);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const f2 v01 = *reinterpret_cast<const f2 *>(s1 + g * kS1Pitch + ao[u]);
                const f2 v23 = *reinterpret_cast<const f2 *>(s1 + g * kS1Pitch + ao[u] + 2);
                acc[u][0] = MFMA4(wa[0], v01[0], acc[u][0]), acc[u][1] = MFMA4(wb[0], v01[0], acc[u][1]);
                acc[u][0] = MFMA4(wa[1], v01[1], acc[u][0]), acc[u][1] = MFMA4(wb[1], v01[1], acc[u][1]);
                acc[u][0] = MFMA4(wa[2], v23[0], acc[u][0]), acc[u][1] = MFMA4(wb[2], v23[0], acc[u][1]);
                acc[u][0] = MFMA4(wa[3], v23[1], acc[u][0]), acc[u][1] = MFMA4(wb[3], v23[1], acc[u][1]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {  // D: channels 16 nb + 4 lk + q x position li
            const int pos = 32 * wave + 16 * u + li;
            if (pos < kP2) {
                float *o = act2 + row * kK3 + 4 * lk * kP2 + pos;
#pragma unroll
                for (int nb = 0; nb < 2; nb++)
#pragma unroll
                    for (int q = 0; q < 4; q++) o[(16 * nb + q) * kP2] = fmaxf(acc[u][nb][q] + bias2[nb][q], 0.f);
            }
        }
        __syncthreads();  // s1 is rewritten by the next row's conv1
    }
}

// ---- conv3 + ReLU: a3[row][oc] = relu(b3[oc] + sum_k act2[row][k] * w3[oc][k]), both operands K-contiguous.  Workgroup tile 128 rows x
// 128 channels, 2 x 2 wavefronts of 64 x 64, K in slabs of 16 through two LDS buffers, k dealt kq-major inside a slab (all as
// policy_full_conv3_kernel); the 242 slabs in 11 segments of 22: a segment accumulates from zero, the segment sums are added in order.
static constexpr int kGM = 128, kGN = 128, kGPitch = 20;  // pitch 20 floats = 5 x 16 bytes, odd: conflict-free 16-lane read phases
static constexpr int kSegSlabs = 22;
__global__ __launch_bounds__(256, 2) void ppo_full_conv3_kernel(const float *__restrict__ act2, const float *__restrict__ w3, const float *__restrict__ b3,
                                                                float *__restrict__ feat, int64_t n) {
    __shared__ __attribute__((aligned(16))) float sA[2][kGM * kGPitch];
    __shared__ __attribute__((aligned(16))) float sB[2][kGN * kGPitch];
    const int64_t m0 = (int64_t)blockIdx.x * kGM;
    const int n0 = blockIdx.y * kGN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4, wm = wave >> 1, wn = wave & 1;
    const int lr = tid >> 2, lc = tid & 3;  // loader: rows lr and lr + 64, 16-byte column lc of the slab
    const float *pa0 = act2 + std::min<int64_t>(m0 + lr, n - 1) * kK3 + 4 * lc;  // rows past the last repeat it (not stored)
    const float *pa1 = act2 + std::min<int64_t>(m0 + lr + 64, n - 1) * kK3 + 4 * lc;
    const float *pb0 = w3 + (int64_t)(n0 + lr) * kK3 + 4 * lc, *pb1 = pb0 + (int64_t)64 * kK3;
    const int so0 = lr * kGPitch + 4 * lc, so1 = so0 + 64 * kGPitch;
    f4 ga0 = *reinterpret_cast<const f4 *>(pa0), ga1 = *reinterpret_cast<const f4 *>(pa1);
    f4 gb0 = *reinterpret_cast<const f4 *>(pb0), gb1 = *reinterpret_cast<const f4 *>(pb1);
    *reinterpret_cast<f4 *>(&sA[0][so0]) = ga0, *reinterpret_cast<f4 *>(&sA[0][so1]) = ga1;
    *reinterpret_cast<f4 *>(&sB[0][so0]) = gb0, *reinterpret_cast<f4 *>(&sB[0][so1]) = gb1;
    __syncthreads();
    f4 acc[4][4], tot[4][4];
#pragma unroll
    for (int mb = 0; mb < 4; mb++)
#pragma unroll
        for (int nb = 0; nb < 4; nb++) acc[mb][nb] = f4{0.f, 0.f, 0.f, 0.f}, tot[mb][nb] = f4{0.f, 0.f, 0.f, 0.f};
    const int ra = (wm * 64 + li) * kGPitch + 4 * lk, rb = (wn * 64 + li) * kGPitch + 4 * lk;
    constexpr int KT = kK3 / 16;  // 242 slabs
    static_assert(KT % kSegSlabs == 0, "whole segments");
    int left = kSegSlabs;
    for (int kt = 0; kt < KT; kt++) {
        const int cur = kt & 1;
        if (kt + 1 < KT) {
            const int o = 16 * (kt + 1);
            ga0 = *reinterpret_cast<const f4 *>(pa0 + o), ga1 = *reinterpret_cast<const f4 *>(pa1 + o);
            gb0 = *reinterpret_cast<const f4 *>(pb0 + o), gb1 = *reinterpret_cast<const f4 *>(pb1 + o);
        }
        f4 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            a[i] = *reinterpret_cast<const f4 *>(&sA[cur][ra + i * 16 * kGPitch]);
            b[i] = *reinterpret_cast<const f4 *>(&sB[cur][rb + i * 16 * kGPitch]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int mb = 0; mb < 4; mb++)
#pragma unroll
                for (int nb = 0; nb < 4; nb++) acc[mb][nb] = MFMA4(a[mb][j], b[nb][j], acc[mb][nb]);
        if (--left == 0) {  // the segment's sum joins the others, the next one starts from zero
            left = kSegSlabs;
#pragma unroll
            for (int mb = 0; mb < 4; mb++)
#pragma unroll
                for (int nb = 0; nb < 4; nb++) tot[mb][nb] += acc[mb][nb], acc[mb][nb] = f4{0.f, 0.f, 0.f, 0.f};
        }
        if (kt + 1 < KT) {
            *reinterpret_cast<f4 *>(&sA[cur ^ 1][so0]) = ga0, *reinterpret_cast<f4 *>(&sA[cur ^ 1][so1]) = ga1;
            *reinterpret_cast<f4 *>(&sB[cur ^ 1][so0]) = gb0, *reinterpret_cast<f4 *>(&sB[cur ^ 1][so1]) = gb1;
        }
        __syncthreads();
    }
#pragma unroll
    for (int nb = 0; nb < 4; nb++) {
        const int oc = n0 + wn * 64 + nb * 16 + li;
        const float bias = b3[oc];
#pragma unroll
        for (int mb = 0; mb < 4; mb++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t row = m0 + wm * 64 + mb * 16 + 4 * lk + q;
                if (row < n) feat[row * kC3 + oc] = fmaxf(tot[mb][nb][q] + bias, 0.f);
            }
    }
}

// ---- heads: a wavefront per row.  TEACHER: include/crl.h "ppo update, teacher targets" -- the row's teacher row and value target are
// fetched at its flat index and the statistics are nine per row.  <false> is what crl_ppo_grad launches, and receives no teacher.
template <bool TEACHER>
__global__ __launch_bounds__(256) void ppo_full_heads_kernel(RolloutView r, const int64_t *__restrict__ idx, int64_t rows, const float *__restrict__ raw,
                                                             const float *__restrict__ a3, float *__restrict__ dz3, float *__restrict__ dh,
                                                             double *__restrict__ stat, std::conditional_t<TEACHER, PpoHyperTeacher, PpoHyperDev> h) {
    constexpr int NS = TEACHER ? kStatAll : kStatN;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *Wa = raw + kOffWa, *Wc = raw + kOffWc;
    float x[4];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int f = lane + 64 * i;
        x[i] = a3[row * kC3 + f];
        const double xd = (double)x[i];
        s0 = fma((double)Wa[f], xd, s0), s1 = fma((double)Wa[kC3 + f], xd, s1), s2 = fma((double)Wa[2 * kC3 + f], xd, s2);
        s3 = fma((double)Wc[f], xd, s3);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s0 += __shfl_xor(s0, d), s1 += __shfl_xor(s1, d), s2 += __shfl_xor(s2, d), s3 += __shfl_xor(s3, d);
    // (a + b and b + a are the same bits: every lane holds the same four sums and forms the same terms)
    const PpoTeacherDev *teacher = nullptr;
    if constexpr (TEACHER) teacher = &h.t;
    const PpoSample sm = sample_scalars(r, sample_of(r, idx, row), teacher);
    const double l[3] = {(double)raw[kOffBa + 0] + s0, (double)raw[kOffBa + 1] + s1, (double)raw[kOffBa + 2] + s2};
    const double v = (double)raw[kOffBc] + s3;
    float dl[3], dv;
    double st[NS];
    ppo_sample_terms<TEACHER>(l, v, sm.act, (double)sm.olp, (double)sm.target, (double)sm.adv, h, teacher, sm.tr, dl, dv, st);
    if (lane == 0) {
        dh[row * 4 + 0] = dl[0], dh[row * 4 + 1] = dl[1], dh[row * 4 + 2] = dl[2], dh[row * 4 + 3] = dv;
#pragma unroll
        for (int k = 0; k < NS; k++) stat[row * NS + k] = st[k];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int f = lane + 64 * i;
        float da3 = Wa[f] * dl[0];
        da3 = __builtin_fmaf(Wa[kC3 + f], dl[1], da3);
        da3 = __builtin_fmaf(Wa[2 * kC3 + f], dl[2], da3);
        da3 = __builtin_fmaf(Wc[f], dv, da3);
        dz3[row * kC3 + f] = x[i] > 0.f ? da3 : 0.f;
    }
}

// acc = add(acc, load(i)) for i = lo .. hi - 1 in order; the loads of 16 terms are issued before their additions (one at a time the
// walk waits a memory latency per term)
template <class T, class Load, class Add>
__device__ __forceinline__ T walk_rows(int64_t lo, int64_t hi, T acc, Load load, Add add) {
    constexpr int U = 16;
    int64_t row = lo;
    for (; row + U <= hi; row += U) {
        decltype(load(row)) v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = load(row + u);
#pragma unroll
        for (int u = 0; u < U; u++) acc = add(acc, v[u]);
    }
    for (; row < hi; row++) acc = add(acc, load(row));
    return acc;
}

// ---- head grad, two levels of a fixed shape.  Slice s = the chunk's rows [256 s, 256 s + 256).  Level one, grid (6, slices): blocks
// x = 0..2 wa[k][c], 3 wc[c], 4 b3[c], 5 threads 0..3 ba / bc and threads 4..8 the statistics; each thread walks its slice's rows in order
// from zero into slot [s][256 x + c] (the statistics: [s][k], float64).  Level two, grid 6: the same thread adds the slices' sums in
// slice order onto the previous chunks' sum (first: onto zero).
// NS: the statistics per row, 5 or the 9 of a teacher gradient (threads 4 .. 4 + NS - 1 of block 5).
static constexpr int kHeadSlice = 256, kHeadSlots = 6 * 256;
template <int NS>
__global__ __launch_bounds__(256) void ppo_full_headslice_kernel(int64_t rows, const float *__restrict__ dh, const float *__restrict__ a3,
                                                                 const float *__restrict__ dz3, const double *__restrict__ stat, float *__restrict__ hs,
                                                                 double *__restrict__ hsd) {
    const int b = blockIdx.x, c = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.y * kHeadSlice, hi = lo + kHeadSlice < rows ? lo + kHeadSlice : rows;
    const auto plus = [](auto acc, auto v) { return acc + v; };
    float *o = hs + (int64_t)blockIdx.y * kHeadSlots + b * 256 + c;
    if (b < 4) {
        *o = walk_rows(lo, hi, 0.f, [&](int64_t row) { return f2{dh[row * 4 + b], a3[row * kC3 + c]}; },
                       [](float acc, f2 v) { return __builtin_fmaf(v[0], v[1], acc); });
    } else if (b == 4) {
        *o = walk_rows(lo, hi, 0.f, [&](int64_t row) { return dz3[row * kC3 + c]; }, plus);
    } else if (c < 4) {
        *o = walk_rows(lo, hi, 0.f, [&](int64_t row) { return dh[row * 4 + c]; }, plus);
    } else if (c < 4 + NS) {
        const int k = c - 4;
        hsd[(int64_t)blockIdx.y * NS + k] = walk_rows(lo, hi, 0.0, [&](int64_t row) { return stat[row * NS + k]; }, plus);
    }
}

template <int NS>
__global__ __launch_bounds__(256) void ppo_full_headsum_kernel(int slices, const float *__restrict__ hs, const double *__restrict__ hsd, float *__restrict__ gacc,
                                                               double *__restrict__ stat_acc, int first) {
    const int b = blockIdx.x, c = threadIdx.x;
    const auto plus = [](auto acc, auto v) { return acc + v; };
    if (b < 5 || c < 4) {
        float *o = gacc + (b < 3 ? kOffWa + b * kC3 + c : b == 3 ? kOffWc + c : b == 4 ? kOffB3 + c : c < 3 ? kOffBa + c : kOffBc);
        *o = walk_rows(0, slices, first ? 0.f : *o, [&](int64_t s) { return hs[s * kHeadSlots + b * 256 + c]; }, plus);
    } else if (c < 4 + NS) {
        const int k = c - 4;
        stat_acc[k] = walk_rows(0, slices, first ? 0.0 : stat_acc[k], [&](int64_t s) { return hsd[s * NS + k]; }, plus);
    }
}

// ---- gW3[oc][n] += sum over the chunk's rows of dz3[row][oc] act2[row][n].  Grid (121, 2): columns n0 = 32 x, channels m0 = 128 y.
__global__ __launch_bounds__(256) void ppo_full_gw3_kernel(const float *__restrict__ dz3, const float *__restrict__ act2, int64_t rows,
                                                           float *__restrict__ gw3, int first) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int m0 = blockIdx.y * 128 + 32 * wave, n0 = blockIdx.x * 32;
    f4 acc[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
#pragma unroll
            for (int q = 0; q < 4; q++)  // D: rows oc = .. + 4 lk + q, cols n = .. + li
                acc[mb][nb][q] = first ? 0.f : gw3[(int64_t)(m0 + 16 * mb + 4 * lk + q) * kK3 + n0 + 16 * nb + li];
    const float *pa = dz3 + m0 + li, *pb = act2 + n0 + li;
    constexpr int U = 4;  // steps in flight: 16 rows' loads are issued before their matrix instructions
    for (int64_t s0 = 0; s0 < rows; s0 += 4 * U) {
        float a[U][2], b[U][2];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t row = s0 + 4 * u + lk;
            const bool ok = row < rows;  // (a row past the chunk is a zero on both sides)
            const int64_t rc = ok ? row : rows - 1;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const float av = pa[rc * kC3 + 16 * q], bv = pb[rc * kK3 + 16 * q];
                a[u][q] = ok ? av : 0.f, b[u][q] = ok ? bv : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int mb = 0; mb < 2; mb++)
#pragma unroll
                for (int nb = 0; nb < 2; nb++) acc[mb][nb] = MFMA4(a[u][mb], b[u][nb], acc[mb][nb]);
    }
#pragma unroll
    for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
#pragma unroll
            for (int q = 0; q < 4; q++) gw3[(int64_t)(m0 + 16 * mb + 4 * lk + q) * kK3 + n0 + 16 * nb + li] = acc[mb][nb][q];
}

// ---- dz2[row][n] = (sum_c dz3[row][c] W3[c][n]) * (act2[row][n] > 0), over act2.  Grid (ceil(rows / 128), 121).
__global__ __launch_bounds__(256) void ppo_full_dz2_kernel(const float *__restrict__ dz3, const float *__restrict__ w3, float *__restrict__ act2,
                                                           int64_t rows) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * 128 + 32 * wave;
    const int n0 = blockIdx.y * 32;
    const float *pa[2];
#pragma unroll
    for (int mb = 0; mb < 2; mb++) pa[mb] = dz3 + std::min<int64_t>(m0 + 16 * mb + li, rows - 1) * kC3 + 4 * lk;  // rows past the last repeat it (not stored)
    const float *pb = w3 + (int64_t)(4 * lk) * kK3 + n0 + li;
    f4 acc[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; mb++) acc[mb][0] = f4{0.f, 0.f, 0.f, 0.f}, acc[mb][1] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int g = 0; g < kC3 / 16; g++) {
        const f4 a0 = *reinterpret_cast<const f4 *>(pa[0] + 16 * g), a1 = *reinterpret_cast<const f4 *>(pa[1] + 16 * g);
        float b[4][2];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int nb = 0; nb < 2; nb++) b[j][nb] = pb[(int64_t)(16 * g + j) * kK3 + 16 * nb];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int nb = 0; nb < 2; nb++) acc[0][nb] = MFMA4(a0[j], b[j][nb], acc[0][nb]), acc[1][nb] = MFMA4(a1[j], b[j][nb], acc[1][nb]);
    }
#pragma unroll
    for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t row = m0 + 16 * mb + 4 * lk + q;
            if (row < rows) {
#pragma unroll
                for (int nb = 0; nb < 2; nb++) {
                    float *p = act2 + row * kK3 + n0 + 16 * nb + li;
                    *p = *p > 0.f ? acc[mb][nb][q] : 0.f;
                }
            }
        }
}

// ---- back: conv2's and conv1's gradients
__global__ __launch_bounds__(256, 1) void ppo_full_back_kernel(RolloutView r, const int64_t *__restrict__ idx, int64_t rows, const float *__restrict__ raw,
                                                               const float *__restrict__ dz2g, float *__restrict__ partials, int first) {
    if ((int64_t)blockIdx.x >= rows) return;  // (the whole workgroup: no row of this chunk, its partial stands)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float *sw = reinterpret_cast<float *>(smem);  // [32][kW2Pitch]
    float *s1 = sw + kC2 * kW2Pitch;              // [16][kS1Pitch]
    float *sdz2 = s1 + kC1 * kS1Pitch;            // [32][kDz2Pitch]
    float *sdz1 = sdz2 + kC2 * kDz2Pitch;         // [16][kDz1Pitch]
    uint8_t *spl = reinterpret_cast<uint8_t *>(sdz1 + kC1 * kDz1Pitch);  // [4][kPlanePad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const float *w2 = raw + kOffW2;
    for (int i = tid; i < kC2 * 64; i += 256) {
        const int rr = i >> 6, c = i & 63;
        *reinterpret_cast<f4 *>(sw + rr * kW2Pitch + 4 * c) = *reinterpret_cast<const f4 *>(w2 + rr * 256 + 4 * c);
    }
    for (int i = tid; i < kC1 * kS1Pitch; i += 256) s1[i] = 0.f;     // the border stays zero
    for (int i = tid; i < kC2 * kDz2Pitch; i += 256) sdz2[i] = 0.f;  // positions 121 .. 124 stay zero
    bf8 wB[3][2];
    conv1_weights(raw + kOffW1, li, lk, wB);
    f4 bias1;
#pragma unroll
    for (int q = 0; q < 4; q++) bias1[q] = raw[kOffB1 + 4 * lk + q];
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f4 accW2[2][4];  // [mb][q]: rows oc2 = 16 mb + 4 lk + ., cols (ic = 4 wave + q, tap = li)
#pragma unroll
    for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int q = 0; q < 4; q++) accW2[mb][q] = zero4;
    f4 accW1 = zero4;           // rows oc1 = 4 lk + ., cols (ic = wave, tap = li)
    float accB2 = 0.f;          // oc2 = tid >> 3, positions (tid & 7) + 8 i
    float accB1 = 0.f;          // oc1 = tid >> 4, positions (tid & 15) + 16 i
    const int ky = li >> 2, kx = li & 3;
    __syncthreads();

    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t flat = sample_of(r, idx, row);
        {  // the planes by the stack rule, the row's dz2
            const SampleAt at = sample_at(r, flat);
            const int depth = r.depth[flat];
            for (int i = tid; i < CRL_POLICY_STACK * kPlaneChunks; i += 256) {
                const int j = i / kPlaneChunks, c = i - j * kPlaneChunks;
                uint4 v{0u, 0u, 0u, 0u};
                if (CRL_POLICY_STACK - 1 - j < depth) v = *plane_of(r, at, j, c);
                reinterpret_cast<uint4 *>(spl)[i] = v;
            }
            const float *src = dz2g + row * kK3;
            for (int i = tid; i < kK3; i += 256) {
                const int c = i / kP2, p = i - c * kP2;
                sdz2[c * kDz2Pitch + p] = src[i];
            }
        }
        conv1_to_lds(r, flat, wB, bias1, s1, wave, li, lk);
        __syncthreads();
        // ---- gW2: step s contracts over positions 4 s + lk (121 .. 123: zeros in dz2, the last position's window in a1)
#pragma unroll 2
        for (int s = 0; s < 31; s++) {
            const int pos = 4 * s + lk, pc = min(pos, kP2 - 1), y = pc / 11, x = pc - 11 * y;
            const float a0 = sdz2[li * kDz2Pitch + pos], a1 = sdz2[(16 + li) * kDz2Pitch + pos];
            const float *bp = s1 + (4 * wave) * kS1Pitch + (2 * y + ky) * kS1Rows + 2 * x + kx;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float bv = bp[q * kS1Pitch];
                accW2[0][q] = MFMA4(a0, bv, accW2[0][q]), accW2[1][q] = MFMA4(a1, bv, accW2[1][q]);
            }
        }
        {  // gb2
            const int oc = tid >> 3;
            for (int p = tid & 7; p < kP2; p += 8) accB2 += sdz2[oc * kDz2Pitch + p];
        }
        // ---- da1 in gather form and dz1: item = (class, tile of 16 of the class's 100 positions), wavefront wave takes items wave, wave + 4, ...
        for (int item = wave; item < 28; item += 4) {
            const int cls = item / 7, tl = item - 7 * cls, py = cls >> 1, px = cls & 1;
            const int q = 16 * tl + li, qc = min(q, 99), yh = qc / 10 + 1, xh = qc - 10 * (yh - 1) + 1;
            const int a = lk >> 1, b = lk & 1;
            const float *ap = sw + li * 16 + (py + 2 * a) * 4 + (px + 2 * b);  // A: W2[oc = s][ic = li][py + 2 a][px + 2 b]
            const float *bp = sdz2 + (yh - a) * 11 + (xh - b);                 // B: dz2[oc = s][yh - a][xh - b]
            f4 da1 = zero4;
#pragma unroll 8
            for (int s = 0; s < kC2; s++) da1 = MFMA4(ap[s * kW2Pitch], bp[s * kDz2Pitch], da1);
            if (q < 100) {  // D: rows ic = 4 lk + ., col = position li of the tile
                const int Yp = 2 * yh + py, Xp = 2 * xh + px;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int ic = 4 * lk + k;
                    sdz1[ic * kDz1Pitch + (Yp - 2) * 20 + (Xp - 2)] = s1[ic * kS1Pitch + Yp * kS1Rows + Xp] > 0.f ? da1[k] : 0.f;
                }
            }
        }
        __syncthreads();
        // ---- gW1: step s contracts over positions 4 s + lk; B = the byte under tap li of plane `wave`, / 255
#pragma unroll 4
        for (int s = 0; s < kP1 / 4; s++) {
            const int pos = 4 * s + lk, y = pos / 20, x = pos - 20 * y;
            const float bv = div255((float)spl[wave * kPlanePad + (2 * y + ky) * kDim + 2 * x + kx]);
            accW1 = MFMA4(sdz1[li * kDz1Pitch + pos], bv, accW1);
        }
        {  // gb1
            const int oc = tid >> 4;
            for (int p = tid & 15; p < kP1; p += 16) accB1 += sdz1[oc * kDz1Pitch + p];
        }
        __syncthreads();  // the row's buffers are free
    }

    // ---- the workgroup's partial blob: written by the first chunk, added to by the later ones
    float *out = partials + (int64_t)blockIdx.x * kBackBlob;
    auto put = [&](int o, float v) { out[o] = first ? v : out[o] + v; };
#pragma unroll
    for (int q = 0; q < 4; q++) put(kOffW1 + (4 * lk + q) * 64 + wave * 16 + li, accW1[q]);  // W1[oc][ic][tap]
#pragma unroll
    for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int k = 0; k < 4; k++) put(kOffW2 + (16 * mb + 4 * lk + k) * 256 + (4 * wave + q) * 16 + li, accW2[mb][q][k]);  // W2[oc][ic][tap]
    accB2 += __shfl_xor(accB2, 1), accB2 += __shfl_xor(accB2, 2), accB2 += __shfl_xor(accB2, 4);
    if ((tid & 7) == 0) put(kOffB2 + (tid >> 3), accB2);
    accB1 += __shfl_xor(accB1, 1), accB1 += __shfl_xor(accB1, 2), accB1 += __shfl_xor(accB1, 4), accB1 += __shfl_xor(accB1, 8);
    if ((tid & 15) == 0) put(kOffB1 + (tid >> 4), accB1);
}

// ---- finish: pong_ppo.h's reduce (elements below kBackBlob from the W partials, the rest from the accumulated sum)
// ... and one workgroup: thread t adds the block sums t, t + 256, ... in order, then the same tree.  out: [0] the sum of squares, [1 .. NS] the means
template <int NS>
__global__ __launch_bounds__(256) void ppo_full_final_kernel(const double *__restrict__ sq_part, const double *__restrict__ stat_acc, int64_t count,
                                                             double *__restrict__ out) {
    __shared__ double s[256];
    double a = 0.0;
    for (int b = threadIdx.x; b < kSqBlocks; b += 256) a += sq_part[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0];
    if (threadIdx.x < NS) out[1 + threadIdx.x] = stat_acc[threadIdx.x] / (double)count;
}

void ppo_full_destroy(PpoFull *f) {
    if (!f) return;
    for (void *q : {(void *)f->act2, (void *)f->a3, (void *)f->dz3, (void *)f->dh, (void *)f->st, (void *)f->gacc, (void *)f->partials, (void *)f->hs, (void *)f->hsd, (void *)f->stat_acc,
                    (void *)f->sq_part})
        if (q) (void)hipFree(q);
    delete f;
}

int64_t ppo_full_scratch_rows(const PpoFull *f) { return f->scratch_rows; }

// TEACHER chooses the instantiations and the statistics' count
template <bool TEACHER>
static int full_grad(::crl_ppo *p, const RolloutView &view, const int64_t *idx_dev, int64_t count,
                     const std::conditional_t<TEACHER, PpoHyperTeacher, PpoHyperDev> &h, hipStream_t st) {
    constexpr int NS = TEACHER ? kStatAll : kStatN;
    PpoFull *f = p->full;
    const int64_t S = f->scratch_rows;
    const int64_t first_rows = std::min(S, count);
    const int groups = (int)std::min<int64_t>(kBackMax, first_rows);  // W: a function of B and scratch_rows alone
    const float *raw = p->raw;
    int first = 1;
    for (int64_t c0 = 0; c0 < count; c0 += S, first = 0) {
        const int64_t rows = std::min(S, count - c0);
        const int64_t *idx = idx_dev + c0;
        hipLaunchKernelGGL(ppo_full_front_kernel, dim3((unsigned)std::min<int64_t>(rows, (int64_t)f->cus * 2)), dim3(256), 0, st, view, idx, rows, raw, f->act2);
        hipLaunchKernelGGL(ppo_full_conv3_kernel, dim3((unsigned)((rows + kGM - 1) / kGM), kC3 / kGN), dim3(256), 0, st, f->act2, raw + kOffW3, raw + kOffB3, f->a3, rows);
        const int slices = (int)((rows + kHeadSlice - 1) / kHeadSlice);
        hipLaunchKernelGGL(ppo_full_heads_kernel<TEACHER>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, view, idx, rows, raw, f->a3, f->dz3, f->dh, f->st, h);
        hipLaunchKernelGGL(ppo_full_headslice_kernel<NS>, dim3(6, slices), dim3(256), 0, st, rows, f->dh, f->a3, f->dz3, f->st, f->hs, f->hsd);
        hipLaunchKernelGGL(ppo_full_headsum_kernel<NS>, dim3(6), dim3(256), 0, st, slices, f->hs, f->hsd, f->gacc, f->stat_acc, first);
        hipLaunchKernelGGL(ppo_full_gw3_kernel, dim3(kK3 / 32, kC3 / 128), dim3(256), 0, st, f->dz3, f->act2, rows, f->gacc + kOffW3, first);
        hipLaunchKernelGGL(ppo_full_dz2_kernel, dim3((unsigned)((rows + 127) / 128), kK3 / 32), dim3(256), 0, st, f->dz3, raw + kOffW3, f->act2, rows);
        hipLaunchKernelGGL(ppo_full_back_kernel, dim3(groups), dim3(256), kBackLds, st, view, idx, rows, raw, f->act2, f->partials, first);
    }
    hipLaunchKernelGGL((ppo_reduce_kernel<kBackBlob, kFullBlob>), dim3(kSqBlocks), dim3(256), 0, st, f->partials, groups, f->gacc, (float)count, p->grad, f->sq_part);
    hipLaunchKernelGGL(ppo_full_final_kernel<NS>, dim3(1), dim3(256), 0, st, f->sq_part, f->stat_acc, count, p->red);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int ppo_full_grad(::crl_ppo *p, const RolloutView &view, const int64_t *idx_dev, int64_t count, const PpoHyperDev &h, const PpoTeacherDev *t,
                  hipStream_t st) {
    return t ? full_grad<true>(p, view, idx_dev, count, PpoHyperTeacher{h, *t}, st) : full_grad<false>(p, view, idx_dev, count, h, st);
}

static void ppo_full_pack(float *blob, const float *const t[10]) {
    memset(blob, 0, (size_t)kFullBlob * sizeof(float));
    policy_full_pack(blob, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    policy_full_pack_critic(blob + kOffWc, t[8], t[9]);
}

}  // namespace crl

using namespace crl;

extern "C" {

int crl_ppo_set_weights_full(crl_ppo *p, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *conv3_w,
                             const float *conv3_b, const float *actor_w, const float *actor_b, const float *critic_w, const float *critic_b) {
    crl_fail_no_ctx();
    if (!p || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !conv3_w || !conv3_b || !actor_w || !actor_b || !critic_w || !critic_b)
        return crl_fail(CRL_EINVAL, "crl_ppo_set_weights_full: null argument (a learner needs its critic)");
    if (!p->full) return crl_fail(CRL_EINVAL, "crl_ppo_set_weights_full: a LightActorCritic learner (crl_ppo_set_weights)");
    std::vector<float> blob(kFullBlob);
    const float *const t[10] = {conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, actor_w, actor_b, critic_w, critic_b};
    ppo_full_pack(blob.data(), t);
    return ppo_upload(p, blob.data());
}

int crl_ppo_create_full(int32_t device, int64_t scratch_rows, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b,
                        const float *conv3_w, const float *conv3_b, const float *actor_w, const float *actor_b, const float *critic_w, const float *critic_b,
                        crl_ppo **out) {
    crl_fail_no_ctx();
    if (!out || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !conv3_w || !conv3_b || !actor_w || !actor_b || !critic_w || !critic_b)
        return crl_fail(CRL_EINVAL, "crl_ppo_create_full: null argument (a learner needs its critic)");
    *out = nullptr;
    if (scratch_rows < 0 || (scratch_rows && scratch_rows < kMinRows) || scratch_rows > kMaxRows)
        return crl_fail(CRL_EINVAL, "crl_ppo_create_full: scratch_rows must be 0 (%lld) or in [%lld, %lld], not %lld", (long long)kDefaultRows, (long long)kMinRows,
                        (long long)kMaxRows,
                        (long long)scratch_rows);
    HIP_TRY(hipSetDevice(device));
    crl_ppo *p = new crl_ppo();
    PpoFull *f = p->full = new PpoFull();
    p->device = device;
    const int64_t S = f->scratch_rows = scratch_rows ? scratch_rows : kDefaultRows;
    if (hipDeviceGetAttribute(&f->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || f->cus <= 0) f->cus = 256;
    const char *who = "crl_ppo_create_full";
    int rc = ppo_alloc(p, kFullBlob, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->gacc, (size_t)kFullBlob * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->act2, (size_t)S * kK3 * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->a3, (size_t)S * kC3 * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->dz3, (size_t)S * kC3 * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->dh, (size_t)S * 4 * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->st, (size_t)S * kStatAll * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->partials, (size_t)kBackMax * kBackBlob * sizeof(float), who);
    const size_t slices = (size_t)((S + kHeadSlice - 1) / kHeadSlice);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->hs, slices * kHeadSlots * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->hsd, slices * kStatAll * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->stat_acc, kStatAll * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&f->sq_part, kSqBlocks * sizeof(double), who);
    if (rc == CRL_OK) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ppo_full_back_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kBackLds);
        if (e != hipSuccess) rc = crl_hip_fail(e, who);
    }
    if (rc == CRL_OK) rc = crl_ppo_set_weights_full(p, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, actor_w, actor_b, critic_w, critic_b);
    if (rc != CRL_OK) {
        crl_ppo_destroy(p);
        return rc;
    }
    *out = p;
    return CRL_OK;
}

int crl_ppo_get_weights_full(crl_ppo *p, float *conv1_w, float *conv1_b, float *conv2_w, float *conv2_b, float *conv3_w, float *conv3_b, float *actor_w,
                             float *actor_b, float *critic_w, float *critic_b) {
    crl_fail_no_ctx();
    if (!p || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !conv3_w || !conv3_b || !actor_w || !actor_b || !critic_w || !critic_b)
        return crl_fail(CRL_EINVAL, "crl_ppo_get_weights_full: null argument");
    if (!p->full) return crl_fail(CRL_EINVAL, "crl_ppo_get_weights_full: a LightActorCritic learner (crl_ppo_get_weights)");
    std::vector<float> blob(kFullBlob);
    if (int rc = ppo_download(p, blob.data())) return rc;
    memcpy(conv1_w, &blob[kOffW1], 1024 * 4), memcpy(conv1_b, &blob[kOffB1], 16 * 4), memcpy(conv2_w, &blob[kOffW2], (size_t)kC2 * 256 * 4);
    memcpy(conv2_b, &blob[kOffB2], kC2 * 4), memcpy(conv3_w, &blob[kOffW3], (size_t)kC3 * kK3 * 4), memcpy(conv3_b, &blob[kOffB3], kC3 * 4);
    memcpy(actor_w, &blob[kOffWa], (size_t)3 * kC3 * 4), memcpy(actor_b, &blob[kOffBa], 3 * 4), memcpy(critic_w, &blob[kOffWc], kC3 * 4);
    critic_b[0] = blob[kOffBc];
    return CRL_OK;
}

}  // extern "C"

// pong_ppo.hip -- the learner's PPO update for the LightActorCritic on the device (include/crl.h "ppo update"): the gradient of the
// clipped-surrogate loss over a minibatch of a crl_rollout, read from the stored uint8 planes, and the clip + Adam step on a master blob
// in the layout of pong_league.h.  Three launches per gradient (gradient, reduce, final) and one per step; nothing touches the host.
// What the other learners share lives here too: the host side of ppo_optim.h (the hyper-parameter check and the blobs' helpers, the
// CarRacing learner's as well) and, with pong_ppo_full.hip, the step kernel; the sample fetch, the loss terms and the reduce kernel of
// both Pong learners are pong_ppo.h's.
//
// The reference ships no trainer (utils/network.py has only the networks): the loss is the written rule of the header.
//
// Gradient kernel.  A workgroup takes groups of eight consecutive idx entries (the group of pong_policy.hip's forward): group w, w + W,
// ... of W = min(256, ceil(B / 8)) workgroups -- a function of B alone.  Per group:
//   stage     the eight samples' four planes, by the stack rule, into LDS (a masked plane as zeros);
//   forward   50 tiles of 16 conv2 positions on v_mfma_f32_16x16x4_f32 exactly as pong_policy_mfma_kernel lays them out (conv1 as four
//             parity classes, conv2 on the accumulators as they stand); relu(conv2) goes to LDS as the features a2 [8][1600];
//   heads     a wavefront per sample: the four dot products over the 1600 features in float64 (lane l: features l, l + 64, ...; then a
//             butterfly), then lane 0 forms the loss terms and dlogits / dv in closed form, float64, rounded once to float32;
//   head grad a thread per feature f = tid + 512 i: gW[k][f] += d[k][e] * a2[e][f], e = 0..7 in order, in registers for the whole launch;
//   backward  the 50 tiles again: conv1 recomputed (its activations for eight samples, 200 KB, do not fit next to the rest),
//             dz2 = (W_heads^T d) * (a2 > 0) per lane in the accumulator layout, then
//               gW2[oc][ic, c]  += dz2[oc][pos] a1_c[ic][pos]          contraction over positions: both operands through a 16 x 16 LDS tile;
//               da1_c^T[pos][ic] = dz2^T[pos][oc] W2[oc][ic][c]        A = dz2's accumulator registers as they stand (rows = pos);
//               gW1[oc][ic, tap] += dz1_c^T[pos][oc] x[pos][ic, tap]   A = dz1^T's registers as they stand, B = bytes / 255 from the planes.
//             Conv2 is 2 x 2 with stride 2, so da1 needs no overlap handling.  gW1 and gW2 are four accumulator tiles each and stay in
//             registers until the workgroup ends; the bias gradients are per-lane sums beside them.
// At the end the eight wavefronts' accumulators are added in wavefront order and the workgroup's partial blob leaves once.
#include <float.h>

#include <type_traits>

#include "crl_internal.h"
#include "pong_league.h"
#include "pong_net.h"
#include "pong_ppo.h"
#include "pong_ring.h"
#include "pong_rollout.h"

namespace crl {

static constexpr int kGE = 8;                        // samples per group
static constexpr int kGPos = 100;                    // 10 x 10 conv2 positions
static constexpr int kGTiles = kGE * kGPos / 16;     // 50
static constexpr int kGWaves = 8;                    // a wavefront per sample in the heads phase
static constexpr int kGThreads = 64 * kGWaves;
static constexpr int kGMaxGroups = 256;              // W <= 256
static constexpr int kFeat = 1600;
static constexpr int kBlob = kLightRawFloats + kLightCriticFloats;  // 8488: the policy blob with its critic tail (pads included, zero)
static constexpr int kHeadIter = (kFeat + kGThreads - 1) / kGThreads;  // 4
static constexpr int kTileStride = 17;               // a 16 x 16 LDS tile, rows padded
static constexpr int kScrWave = 5 * 16 * kTileStride;  // per wavefront: a1 of the four classes, dz2

static constexpr int kLdsBuf = kGE * CRL_POLICY_STACK * kPlanePad;       // 56 832
static constexpr int kLdsA2 = kGE * kFeat * 4;                           // 51 200
static constexpr int kLdsScr = kGWaves * kScrWave * 4;                   // 43 520
static constexpr int kLdsSmall = (kGE * 4 + kGE * 4) * 4 + kGE * kStatN * 8;
static constexpr int kLdsGrad = kLdsBuf + kLdsA2 + kLdsScr + kLdsSmall;
static constexpr int kRedWave = 2048 + 32;  // a wavefront's gW1, gW2, gb1, gb2 on their way out
static_assert(kGWaves == kGE, "the heads phase gives a wavefront to a sample");
static_assert(kLdsGrad <= 160 * 1024, "the gradient kernel's LDS must fit a CU");
static_assert(kGWaves * kRedWave * 4 <= kLdsBuf + kLdsA2, "the final reduction reuses the staging buffers");
// the teacher instantiation: nine statistics per sample, and behind them the samples' teacher rows [kGE][4] (three logits, the label)
static constexpr int kLdsGradTeacher = kLdsGrad + kGE * kStatT * 8 + kGE * 4 * 4;
static_assert(kLdsGradTeacher <= 160 * 1024, "the teacher gradient kernel's LDS must fit a CU");

struct GradArgs {
    RolloutView r;
    const int64_t *idx;
    int64_t count;
    const float *raw;    // the learner's master blob
    float *partials;     // [W][kBlob]
    double *stat_part;   // [W][kStatN]
    PpoHyperDev h;
};
struct GradArgsTeacher : GradArgs {  // (built as GradArgsTeacher{a, t})
    PpoTeacherDev t;
};

// the wavefront's own LDS traffic in program order (a tile is written by some lanes and read by others)
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// TEACHER: include/crl.h "ppo update, teacher targets" -- the staging also keeps the samples' teacher rows (the value target is the
// teacher's where it has one), the heads phase forms the teacher term and the statistics are nine.  <false> is what crl_ppo_grad launches.
template <bool TEACHER>
__global__ __launch_bounds__(kGThreads, 1) void pong_ppo_grad_kernel(std::conditional_t<TEACHER, GradArgsTeacher, GradArgs> a) {
    constexpr int NS = TEACHER ? kStatAll : kStatN;
    const PpoTeacherDev *teacher = nullptr;
    if constexpr (TEACHER) teacher = &a.t;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *sh_buf = smem;                                                  // [kGE][4][kPlanePad]
    float *sh_a2 = reinterpret_cast<float *>(smem + kLdsBuf);               // [kGE][1600]
    float *sh_scr = sh_a2 + kGE * kFeat;                                     // [kGWaves][5][16][17]
    float *sh_dh = sh_scr + kGWaves * kScrWave;                              // [kGE][4]: dlogits, dv
    float *sh_sc = sh_dh + kGE * 4;                                          // [kGE][4]: action, old log-prob, return, advantage
    double *sh_st = reinterpret_cast<double *>(sh_sc + kGE * 4);             // [kGE][NS]
    [[maybe_unused]] float *sh_tr = reinterpret_cast<float *>(sh_st + kGE * NS);  // (TEACHER) [kGE][4]: teacher logits, label
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lj = lane & 15, lk = lane >> 4;
    const int64_t ngroups = (a.count + kGE - 1) / kGE;
    const float *W1 = a.raw + kLightW1, *W2 = a.raw + kLightW2, *Wa = a.raw + kLightWa, *Wc = a.raw + kLightWc;

    // the wavefront's weights, once.  conv1 A: W1[oc = lj][ic = lk][tap s]; conv2 A: W2[oc2 = lj][ic = 4 lk + r][c];
    // da1 B: W2[oc2 = 4 lk + r][ic = lj][c]
    float w1[16], w2[4][4], w2b[4][4];
#pragma unroll
    for (int s = 0; s < 16; s++) w1[s] = W1[lj * 64 + lk * 16 + s];
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) w2[c][r] = W2[(lj * 16 + 4 * lk + r) * 4 + c], w2b[c][r] = W2[((4 * lk + r) * 16 + lj) * 4 + c];
    f4 bias1, bias2;
#pragma unroll
    for (int r = 0; r < 4; r++) bias1[r] = a.raw[kLightB1 + 4 * lk + r], bias2[r] = a.raw[kLightB2 + 4 * lk + r];

    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f4 accW1[4] = {zero4, zero4, zero4, zero4};  // [ic]: rows oc1 = 4 lk + r, cols tap = lj
    f4 accW2[4] = {zero4, zero4, zero4, zero4};  // [c]: rows oc2 = 4 lk + r, cols ic = lj
    f4 accB2 = zero4;                            // rows oc2 = 4 lk + r, this lane's positions
    float accB1 = 0.f;                           // oc1 = lj, this lane's positions
    float gWh[4][kHeadIter];                     // heads k (actor 0..2, critic), feature tid + 512 i
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int i = 0; i < kHeadIter; i++) gWh[k][i] = 0.f;
    float gbh[4] = {0.f, 0.f, 0.f, 0.f};         // (thread 0)
    double wst[NS] = {};                         // (thread 0)
    float *scr = sh_scr + wave * kScrWave;

    // a lane's 6 x 6 patch of plane ic = lk under conv2 position q of the group, as x / 255
    auto gather = [&](int t, float(&xo)[6][6]) {
        const int q = 16 * t + lj, e = q / kGPos, pos = q - e * kGPos, y2 = pos / 10, x2 = pos - y2 * 10;
        const uint8_t *base = sh_buf + (e * CRL_POLICY_STACK + lk) * kPlanePad + (4 * y2) * kDim + 4 * x2;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const uint32_t *p32 = reinterpret_cast<const uint32_t *>(base + r * kDim - 2 * (r & 1));
            uint32_t w0 = p32[0], w1_ = p32[1];
            if (r & 1) w0 = (w0 >> 16) | (w1_ << 16), w1_ >>= 16;
            const float b[6] = {(float)(w0 & 255u), (float)((w0 >> 8) & 255u), (float)((w0 >> 16) & 255u), (float)(w0 >> 24),
                                (float)(w1_ & 255u), (float)((w1_ >> 8) & 255u)};
#pragma unroll
            for (int k = 0; k < 6; k++) xo[r][k] = div255(b[k]);
        }
    };
    auto conv1 = [&](const float(&xin)[6][6], f4(&d1)[4]) {
#pragma unroll
        for (int c = 0; c < 4; c++) d1[c] = bias1;
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
            for (int c = 0; c < 4; c++)
                d1[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], xin[2 * (c >> 1) + (s >> 2)][2 * (c & 1) + (s & 3)], d1[c], 0, 0, 0);
    };

    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b0 = g * kGE;
        const int here = (int)((a.count - b0) < kGE ? (a.count - b0) : kGE);
        // ---- stage: planes by the stack rule, scalars
        for (int i = tid; i < kGE * CRL_POLICY_STACK * kPlaneChunks; i += kGThreads) {
            const int fe = i / (CRL_POLICY_STACK * kPlaneChunks), rem = i - fe * (CRL_POLICY_STACK * kPlaneChunks);
            const int j = rem / kPlaneChunks, c = rem - j * kPlaneChunks;
            uint4 v{0u, 0u, 0u, 0u};
            if (fe < here) {
                const uint32_t flat = sample_of(a.r, a.idx, b0 + fe);
                if (CRL_POLICY_STACK - 1 - j < (int)a.r.depth[flat]) v = *plane_of(a.r, sample_at(a.r, flat), j, c);
            }
            reinterpret_cast<uint4 *>(sh_buf)[(fe * CRL_POLICY_STACK + j) * kPlaneChunks + c] = v;
        }
        if (tid < kGE) {
            PpoSample sm;
            if (tid < here) sm = sample_scalars(a.r, sample_of(a.r, a.idx, b0 + tid), teacher);
            sh_sc[tid * 4 + 0] = (float)sm.act, sh_sc[tid * 4 + 1] = sm.olp, sh_sc[tid * 4 + 2] = sm.target, sh_sc[tid * 4 + 3] = sm.adv;
            if constexpr (TEACHER) {
                sh_tr[tid * 4 + 0] = sm.tr.l[0], sh_tr[tid * 4 + 1] = sm.tr.l[1], sh_tr[tid * 4 + 2] = sm.tr.l[2];
                reinterpret_cast<int32_t *>(sh_tr)[tid * 4 + 3] = sm.tr.label;
            }
        }
        __syncthreads();
        // ---- forward: the features
        for (int t = wave; t < kGTiles; t += kGWaves) {
            const int q = 16 * t + lj, e = q / kGPos, pos = q - e * kGPos;
            float xin[6][6];
            gather(t, xin);
            f4 d1[4];
            conv1(xin, d1);
            f4 d2a = bias2, d2b = zero4;
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float hval = fmaxf(d1[c][r], 0.f);
                    if ((c * 4 + r) & 1) d2b = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[c][r], hval, d2b, 0, 0, 0);
                    else d2a = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[c][r], hval, d2a, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; r++) sh_a2[e * kFeat + (4 * lk + r) * kGPos + pos] = fmaxf(d2a[r] + d2b[r], 0.f);
        }
        __syncthreads();
        // ---- heads: wavefront e = sample e
        {
            const int e = wave;
            // float64 from here to dlogits / dv: the head sums are long and cancel (sum |w a| is a hundred times |v| on dense frames), and a
            // sample's whole gradient hangs on v - ret and on logp - old_logp; 6 400 double multiply-adds per sample beside 1 500 MFMAs
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int i = 0; i < kFeat / 64; i++) {
                const int f = lane + 64 * i;
                const double x = (double)sh_a2[e * kFeat + f];
                s0 = fma((double)Wa[f], x, s0), s1 = fma((double)Wa[kFeat + f], x, s1), s2 = fma((double)Wa[2 * kFeat + f], x, s2);
                s3 = fma((double)Wc[f], x, s3);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s0 += __shfl_xor(s0, d), s1 += __shfl_xor(s1, d), s2 += __shfl_xor(s2, d), s3 += __shfl_xor(s3, d);
            if (lane == 0) {
                float dl[3] = {0.f, 0.f, 0.f}, dv = 0.f;
                double st[NS] = {};
                if (e < here) {
                    const double l[3] = {(double)a.raw[kLightBa + 0] + s0, (double)a.raw[kLightBa + 1] + s1, (double)a.raw[kLightBa + 2] + s2};
                    const double v = (double)a.raw[kLightBc] + s3;
                    const int act = (int)sh_sc[e * 4 + 0];
                    const double olp = (double)sh_sc[e * 4 + 1], ret = (double)sh_sc[e * 4 + 2], A = (double)sh_sc[e * 4 + 3];
                    TeacherRow tr;
                    if constexpr (TEACHER) tr = TeacherRow{{sh_tr[e * 4 + 0], sh_tr[e * 4 + 1], sh_tr[e * 4 + 2]}, reinterpret_cast<const int32_t *>(sh_tr)[e * 4 + 3]};
                    ppo_sample_terms<TEACHER>(l, v, act, olp, ret, A, a.h, teacher, tr, dl, dv, st);
                }
                sh_dh[e * 4 + 0] = dl[0], sh_dh[e * 4 + 1] = dl[1], sh_dh[e * 4 + 2] = dl[2], sh_dh[e * 4 + 3] = dv;
#pragma unroll
                for (int k = 0; k < NS; k++) sh_st[e * NS + k] = st[k];
            }
        }
        __syncthreads();
        // ---- the heads' gradients: samples in order
#pragma unroll
        for (int i = 0; i < kHeadIter; i++) {
            const int f = tid + kGThreads * i;
            if (f < kFeat) {
#pragma unroll
                for (int e = 0; e < kGE; e++) {
                    const float x = sh_a2[e * kFeat + f];
#pragma unroll
                    for (int k = 0; k < 4; k++) gWh[k][i] = __builtin_fmaf(sh_dh[e * 4 + k], x, gWh[k][i]);
                }
            }
        }
        if (tid == 0) {
            for (int e = 0; e < kGE; e++) {
#pragma unroll
                for (int k = 0; k < 4; k++) gbh[k] += sh_dh[e * 4 + k];
#pragma unroll
                for (int k = 0; k < NS; k++) wst[k] += sh_st[e * NS + k];
            }
        }
        // ---- backward through the convolutions
        for (int t = wave; t < kGTiles; t += kGWaves) {
            const int q = 16 * t + lj, e = q / kGPos, pos = q - e * kGPos;
            float xin[6][6];
            gather(t, xin);
            f4 d1[4];
            conv1(xin, d1);
            f4 dz2;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int f = (4 * lk + r) * kGPos + pos;
                float da2 = Wa[f] * sh_dh[e * 4 + 0];
                da2 = __builtin_fmaf(Wa[kFeat + f], sh_dh[e * 4 + 1], da2);
                da2 = __builtin_fmaf(Wa[2 * kFeat + f], sh_dh[e * 4 + 2], da2);
                da2 = __builtin_fmaf(Wc[f], sh_dh[e * 4 + 3], da2);
                dz2[r] = sh_a2[e * kFeat + f] > 0.f ? da2 : 0.f;
            }
            accB2 += dz2;
            wave_lds_sync();  // (the tile before this one has been read)
#pragma unroll
            for (int r = 0; r < 4; r++) {
#pragma unroll
                for (int c = 0; c < 4; c++) scr[(c * 16 + 4 * lk + r) * kTileStride + lj] = fmaxf(d1[c][r], 0.f);
                scr[(64 + 4 * lk + r) * kTileStride + lj] = dz2[r];
            }
            wave_lds_sync();
            // gW2[oc2][ic][c] += sum_pos dz2[oc2][pos] a1_c[ic][pos]: step s contracts over positions 4 s + lk
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const float av = scr[(64 + lj) * kTileStride + 4 * s + lk];
#pragma unroll
                for (int c = 0; c < 4; c++)
                    accW2[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, scr[(c * 16 + lj) * kTileStride + 4 * s + lk], accW2[c], 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < 4; c++) {
                // da1_c^T[pos][ic]: step r contracts over oc2 = 4 lk + r.  D: rows pos = 4 lk + r', cols ic = lj
                f4 da1 = zero4;
#pragma unroll
                for (int r = 0; r < 4; r++) da1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dz2[r], w2b[c][r], da1, 0, 0, 0);
                f4 dz1;
#pragma unroll
                for (int r = 0; r < 4; r++) dz1[r] = scr[(c * 16 + lj) * kTileStride + 4 * lk + r] > 0.f ? da1[r] : 0.f;
                accB1 += (dz1[0] + dz1[1]) + (dz1[2] + dz1[3]);
                // gW1[oc1][ic][tap] += sum_pos dz1^T[pos][oc1] x[pos][ic][tap]: step r contracts over positions 4 lk + r; B = the byte of
                // position 4 lk + r under tap lj of class c, / 255
                const int ky = lj >> 2, kx = lj & 3;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int q1 = 16 * t + 4 * lk + r, e1 = q1 / kGPos, p1 = q1 - e1 * kGPos, y2 = p1 / 10, x2 = p1 - y2 * 10;
                    const uint8_t *px = sh_buf + e1 * (CRL_POLICY_STACK * kPlanePad) + (4 * y2 + 2 * (c >> 1) + ky) * kDim + 4 * x2 + 2 * (c & 1) + kx;
#pragma unroll
                    for (int ic = 0; ic < 4; ic++)
                        accW1[ic] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz1[r], div255((float)px[ic * kPlanePad]), accW1[ic], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);  // (a class at a time: the 64 byte loads of a tile hoisted together spill)
            }
        }
        __syncthreads();  // the group's buffers are free
    }

    // ---- the workgroup's partial blob: the wavefronts' accumulators in wavefront order
    float *red = reinterpret_cast<float *>(smem) + wave * kRedWave;
#pragma unroll
    for (int ic = 0; ic < 4; ic++)
#pragma unroll
        for (int r = 0; r < 4; r++) red[(4 * lk + r) * 64 + ic * 16 + lj] = accW1[ic][r];         // W1[oc][ic][tap]
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) red[1024 + ((4 * lk + r) * 16 + lj) * 4 + c] = accW2[c][r];   // W2[oc][ic][c]
    accB1 += __shfl_xor(accB1, 16), accB1 += __shfl_xor(accB1, 32);
#pragma unroll
    for (int d = 1; d <= 8; d <<= 1)
#pragma unroll
        for (int r = 0; r < 4; r++) accB2[r] += __shfl_xor(accB2[r], d);
    if (lk == 0) red[2048 + lj] = accB1;
    if (lj == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) red[2048 + 16 + 4 * lk + r] = accB2[r];
    }
    __syncthreads();
    float *out = a.partials + (int64_t)blockIdx.x * kBlob;
    const float *red0 = reinterpret_cast<const float *>(smem);
    for (int i = tid; i < kRedWave; i += kGThreads) {
        float s = red0[i];
#pragma unroll
        for (int w = 1; w < kGWaves; w++) s += red0[w * kRedWave + i];
        const int o = i < 1024 ? kLightW1 + i : i < 2048 ? kLightW2 + (i - 1024) : i < 2048 + 16 ? kLightB1 + (i - 2048) : kLightB2 + (i - 2048 - 16);
        out[o] = s;
    }
#pragma unroll
    for (int i = 0; i < kHeadIter; i++) {
        const int f = tid + kGThreads * i;
        if (f < kFeat) out[kLightWa + f] = gWh[0][i], out[kLightWa + kFeat + f] = gWh[1][i], out[kLightWa + 2 * kFeat + f] = gWh[2][i], out[kLightWc + f] = gWh[3][i];
    }
    if (tid == 0) {
        out[kLightBa + 0] = gbh[0], out[kLightBa + 1] = gbh[1], out[kLightBa + 2] = gbh[2], out[kLightBa + 3] = 0.f;
        out[kLightBc + 0] = gbh[3], out[kLightBc + 1] = 0.f, out[kLightBc + 2] = 0.f, out[kLightBc + 3] = 0.f;
#pragma unroll
        for (int k = 0; k < NS; k++) a.stat_part[blockIdx.x * NS + k] = wst[k];
    }
}

static constexpr int kRedBlocks = (kBlob + 255) / 256;  // 34
// ... and one lane: the 34 sums of squares in order, the W statistics partials in order.  out: [0] the sum of squares, [1 .. NS] the means
// (NS = 5, or the 9 of a teacher gradient)
template <int NS>
__global__ void pong_ppo_final_kernel(const double *__restrict__ sq_part, const double *__restrict__ stat_part, int groups, int64_t count,
                                      double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sq = 0.0;
    for (int b = 0; b < kRedBlocks; b++) sq += sq_part[b];
    out[0] = sq;
    for (int k = 0; k < NS; k++) {
        double s = 0.0;
        for (int w = 0; w < groups; w++) s += stat_part[w * NS + k];
        out[1 + k] = s / (double)count;
    }
}

struct StepArgs {
    AdamBlobs b;
    const double *red;  // [0]: the gradient's sum of squares
    AdamArgs h;
    int n;  // the blob's floats
};

// include/crl.h "ppo update", optimiser step, over a blob of a.n floats (either learner's)
__global__ __launch_bounds__(256) void pong_ppo_step_kernel(StepArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    a.b.raw[i] = adam_lane(a.h, a.b, i, a.red[0]);
}

// ---- ppo_optim.h's host side, every learner's
int ppo_hyper_check(const char *who, const crl_ppo_hyper *h) {
    if (!h) return crl_fail(CRL_EINVAL, "%s: null hyper-parameters", who);
    if (!(h->clip >= 0.f) || !(h->lr >= 0.f) || !(h->beta1 >= 0.f && h->beta1 < 1.f) || !(h->beta2 >= 0.f && h->beta2 < 1.f) || !(h->eps > 0.f) ||
        !(h->max_grad_norm > 0.f) || !(h->vf_coef == h->vf_coef) || !(h->ent_coef == h->ent_coef))
        return crl_fail(CRL_EINVAL, "%s: clip >= 0, lr >= 0, betas in [0, 1), eps > 0, max_grad_norm > 0, no NaN", who);
    return CRL_OK;
}

int ppo_alloc_blobs(PpoBlobs *p, int blob_floats, const char *who) {
    p->blob_floats = blob_floats;
    int rc = CRL_OK;
    for (float **q : {&p->raw, &p->m, &p->v, &p->grad})
        if (rc == CRL_OK) rc = crl_dev_zalloc(q, (size_t)blob_floats * sizeof(float), who);
    return rc;
}

void ppo_free_blobs(PpoBlobs *p) {
    for (float *q : {p->raw, p->m, p->v, p->grad})
        if (q) (void)hipFree(q);
}

int ppo_alloc(::crl_ppo *p, int blob_floats, const char *who) {
    const int rc = ppo_alloc_blobs(p, blob_floats, who);
    return rc != CRL_OK ? rc : crl_dev_zalloc(&p->red, (1 + kStatAll) * sizeof(double), who);
}

int ppo_read_grad(PpoBlobs *p, const float **grad_dev, float *grad_out_host) {
    if (grad_dev) *grad_dev = p->grad;
    if (grad_out_host) {
        HIP_TRY(hipSetDevice(p->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(grad_out_host, p->grad, (size_t)p->blob_floats * sizeof(float), hipMemcpyDeviceToHost));
    }
    return CRL_OK;
}

int ppo_read_state(PpoBlobs *p, float *blob_out_host, float *m_out_host, float *v_out_host, int64_t *steps_out, hipStream_t st) {
    const size_t bytes = (size_t)p->blob_floats * sizeof(float);
    HIP_TRY(hipSetDevice(p->device));
    if (blob_out_host) HIP_TRY(hipMemcpyAsync(blob_out_host, p->raw, bytes, hipMemcpyDeviceToHost, st));
    if (m_out_host) HIP_TRY(hipMemcpyAsync(m_out_host, p->m, bytes, hipMemcpyDeviceToHost, st));
    if (v_out_host) HIP_TRY(hipMemcpyAsync(v_out_host, p->v, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (steps_out) *steps_out = p->steps;
    return CRL_OK;
}

int ppo_write_state(PpoBlobs *p, const float *blob_host, const float *m_host, const float *v_host, int64_t steps, hipStream_t st) {
    const size_t bytes = (size_t)p->blob_floats * sizeof(float);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(p->raw, blob_host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p->m, m_host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p->v, v_host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    p->steps = steps, p->have_grad = false;
    return CRL_OK;
}

int ppo_upload(PpoBlobs *p, const float *blob) {
    const size_t bytes = (size_t)p->blob_floats * sizeof(float);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(p->raw, blob, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(p->m, 0, bytes));
    HIP_TRY(hipMemset(p->v, 0, bytes));
    HIP_TRY(hipDeviceSynchronize());
    p->steps = 0;
    return CRL_OK;
}

int ppo_download(PpoBlobs *p, float *blob) {
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(blob, p->raw, (size_t)p->blob_floats * sizeof(float), hipMemcpyDeviceToHost));
    return CRL_OK;
}

}  // namespace crl

using namespace crl;

static void ppo_pack(float *blob, const float *const t[8]) {
    for (int i = 0; i < kBlob; i++) blob[i] = 0.f;
    policy_light_pack(blob, t[0], t[1], t[2], t[3], t[4], t[5]);
    policy_light_pack_critic(blob + kLightWc, t[6], t[7]);
}

// the light learner's three launches; TEACHER chooses the instantiations, their LDS and the statistics' count
template <bool TEACHER>
static int ppo_light_grad(crl_ppo *p, const std::conditional_t<TEACHER, GradArgsTeacher, GradArgs> &a, hipStream_t st) {
    const int64_t ngroups = (a.count + kGE - 1) / kGE;
    const int groups = (int)(ngroups < kGMaxGroups ? ngroups : kGMaxGroups);
    hipLaunchKernelGGL(pong_ppo_grad_kernel<TEACHER>, dim3(groups), dim3(kGThreads), TEACHER ? kLdsGradTeacher : kLdsGrad, st, a);
    hipLaunchKernelGGL((ppo_reduce_kernel<kBlob, kBlob>), dim3(kRedBlocks), dim3(256), 0, st, p->partials, groups, nullptr, (float)a.count, p->grad, p->sq_part);
    hipLaunchKernelGGL(pong_ppo_final_kernel<TEACHER ? kStatAll : kStatN>, dim3(1), dim3(64), 0, st, p->sq_part, p->stat_part, groups, a.count, p->red);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

extern "C" {

void crl_ppo_destroy(crl_ppo *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    ppo_full_destroy(p->full);
    ppo_free_blobs(p);
    for (void *q : {(void *)p->partials, (void *)p->stat_part, (void *)p->sq_part, (void *)p->red})
        if (q) (void)hipFree(q);
    delete p;
}

int crl_ppo_set_weights(crl_ppo *p, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *actor_w,
                        const float *actor_b, const float *critic_w, const float *critic_b) {
    crl_fail_no_ctx();
    if (!p || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b || !critic_w || !critic_b)
        return crl_fail(CRL_EINVAL, "crl_ppo_set_weights: null argument (a learner needs its critic)");
    if (p->full) return crl_fail(CRL_EINVAL, "crl_ppo_set_weights: a full-size learner (crl_ppo_set_weights_full)");
    std::vector<float> blob(kBlob);
    const float *const t[8] = {conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b, critic_w, critic_b};
    ppo_pack(blob.data(), t);
    return ppo_upload(p, blob.data());
}

int crl_ppo_create(int32_t device, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *actor_w,
                   const float *actor_b, const float *critic_w, const float *critic_b, crl_ppo **out) {
    crl_fail_no_ctx();
    if (!out || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b || !critic_w || !critic_b)
        return crl_fail(CRL_EINVAL, "crl_ppo_create: null argument (a learner needs its critic)");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    crl_ppo *p = new crl_ppo();
    p->device = device;
    const char *who = "crl_ppo_create";
    int rc = ppo_alloc(p, kBlob, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->partials, (size_t)kGMaxGroups * kBlob * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->stat_part, (size_t)kGMaxGroups * kStatAll * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->sq_part, kRedBlocks * sizeof(double), who);
    if (rc == CRL_OK) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pong_ppo_grad_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsGrad);
        if (e != hipSuccess) rc = crl_hip_fail(e, who);
    }
    if (rc == CRL_OK) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pong_ppo_grad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsGradTeacher);
        if (e != hipSuccess) rc = crl_hip_fail(e, who);
    }
    if (rc == CRL_OK) rc = crl_ppo_set_weights(p, conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b, critic_w, critic_b);
    if (rc != CRL_OK) {
        crl_ppo_destroy(p);
        return rc;
    }
    *out = p;
    return CRL_OK;
}

int crl_ppo_get_weights(crl_ppo *p, float *conv1_w, float *conv1_b, float *conv2_w, float *conv2_b, float *actor_w, float *actor_b, float *critic_w,
                        float *critic_b) {
    crl_fail_no_ctx();
    if (!p || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b || !critic_w || !critic_b)
        return crl_fail(CRL_EINVAL, "crl_ppo_get_weights: null argument");
    if (p->full) return crl_fail(CRL_EINVAL, "crl_ppo_get_weights: a full-size learner (crl_ppo_get_weights_full)");
    std::vector<float> blob(kBlob);
    if (int rc = ppo_download(p, blob.data())) return rc;
    memcpy(conv1_w, &blob[kLightW1], 1024 * 4), memcpy(conv1_b, &blob[kLightB1], 16 * 4), memcpy(conv2_w, &blob[kLightW2], 1024 * 4);
    memcpy(conv2_b, &blob[kLightB2], 16 * 4), memcpy(actor_w, &blob[kLightWa], 4800 * 4), memcpy(actor_b, &blob[kLightBa], 3 * 4);
    memcpy(critic_w, &blob[kLightWc], 1600 * 4), critic_b[0] = blob[kLightBc];
    return CRL_OK;
}

int crl_ppo_weights_dev(crl_ppo *p, const float **blob_dev) {
    crl_fail_no_ctx();
    if (!p || !blob_dev) return crl_fail(CRL_EINVAL, "crl_ppo_weights_dev: null argument");
    *blob_dev = p->raw;
    return CRL_OK;
}

// crl_ppo_grad (teacher null) and crl_ppo_grad_teacher: everything is looked at before the learner or the GPU is touched
static int ppo_grad(const char *who, crl_ppo *p, const crl_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper,
                    const crl_ppo_teacher *teacher, void *stream) {
    crl_fail_no_ctx();
    if (!p || !rollout || !idx_dev) return crl_fail(CRL_EINVAL, "%s: null argument", who);
    if ((uintptr_t)idx_dev & 7) return crl_fail(CRL_EINVAL, "%s: idx must be 8-byte aligned", who);
    if (count < 1 || count > 0x7fffffff) return crl_fail(CRL_EINVAL, "%s: the number of samples must be in [1, 2^31)", who);
    if (int rc = ppo_hyper_check(who, hyper)) return rc;
    const RolloutView view = rollout_view(rollout);
    if (!view.finished) return crl_fail(CRL_EINVAL, "%s: the rollout is not finished (crl_rollout_finish computes returns and advantages)", who);
    PpoTeacherDev t{};
    if (teacher) {
        if (!teacher->logits_dev == !teacher->labels_dev) return crl_fail(CRL_EINVAL, "%s: a teacher has logits or labels, exactly one of the two", who);
        if (teacher->rows != (int64_t)view.last + 1)
            return crl_fail(CRL_EINVAL, "%s: the teacher holds %lld rows, the rollout's T * N is %lld", who, (long long)teacher->rows, (long long)view.last + 1);
        if (!(teacher->temperature > 0.f && teacher->temperature <= FLT_MAX)) return crl_fail(CRL_EINVAL, "%s: the temperature must be finite and > 0", who);
        if (!(teacher->coef >= 0.f && teacher->coef <= FLT_MAX)) return crl_fail(CRL_EINVAL, "%s: coef must be finite and >= 0", who);
        if (teacher->policy_term != 0 && teacher->policy_term != 1)
            return crl_fail(CRL_EINVAL, "%s: policy_term must be 0 or 1, not %d", who, (int)teacher->policy_term);
        if (((uintptr_t)teacher->logits_dev | (uintptr_t)teacher->labels_dev | (uintptr_t)teacher->value_targets_dev) & 3)
            return crl_fail(CRL_EINVAL, "%s: the teacher's arrays must be 4-byte aligned", who);
        t = PpoTeacherDev{teacher->logits_dev, teacher->labels_dev, teacher->value_targets_dev, teacher->temperature, teacher->coef, teacher->policy_term};
    }
    hipStream_t st = (hipStream_t)stream;
    const PpoHyperDev h{hyper->clip, hyper->vf_coef, hyper->ent_coef};
    int rc;
    if (p->full) {
        rc = ppo_full_grad(p, view, idx_dev, count, h, teacher ? &t : nullptr, st);
    } else {
        const GradArgs a{view, idx_dev, count, p->raw, p->partials, p->stat_part, h};
        rc = teacher ? ppo_light_grad<true>(p, GradArgsTeacher{a, t}, st) : ppo_light_grad<false>(p, a, st);
    }
    if (rc) return rc;
    p->have_grad = true, p->teacher_grad = teacher != nullptr;
    return CRL_OK;
}

int crl_ppo_grad(crl_ppo *p, const crl_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper, void *stream) {
    return ppo_grad("crl_ppo_grad", p, rollout, idx_dev, count, hyper, nullptr, stream);
}

int crl_ppo_grad_teacher(crl_ppo *p, const crl_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper,
                         const crl_ppo_teacher *teacher, void *stream) {
    crl_fail_no_ctx();
    if (!teacher) return crl_fail(CRL_EINVAL, "crl_ppo_grad_teacher: null teacher (crl_ppo_grad is the plain gradient)");
    return ppo_grad("crl_ppo_grad_teacher", p, rollout, idx_dev, count, hyper, teacher, stream);
}

int crl_ppo_get_grad(crl_ppo *p, const float **grad_dev, float *grad_out_host) {
    crl_fail_no_ctx();
    if (!p || (!grad_dev && !grad_out_host)) return crl_fail(CRL_EINVAL, "crl_ppo_get_grad: null argument");
    if (!p->have_grad) return crl_fail(CRL_EINVAL, "crl_ppo_get_grad: no gradient yet (crl_ppo_grad)");
    return ppo_read_grad(p, grad_dev, grad_out_host);
}

int crl_ppo_step(crl_ppo *p, const crl_ppo_hyper *hyper, void *stream) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_ppo_step: null learner");
    if (int rc = ppo_hyper_check("crl_ppo_step", hyper)) return rc;
    if (!p->have_grad) return crl_fail(CRL_EINVAL, "crl_ppo_step: no gradient yet (crl_ppo_grad)");
    const int64_t t = p->steps + 1;
    const StepArgs a{p->adam(), p->red, adam_args(hyper, t), p->blob_floats};
    hipLaunchKernelGGL(pong_ppo_step_kernel, dim3((p->blob_floats + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    p->steps = t;
    return CRL_OK;
}

int crl_ppo_stats(crl_ppo *p, double *out7_host) {
    crl_fail_no_ctx();
    if (!p || !out7_host) return crl_fail(CRL_EINVAL, "crl_ppo_stats: null argument");
    if (!p->have_grad) return crl_fail(CRL_EINVAL, "crl_ppo_stats: no gradient yet (crl_ppo_grad)");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    double red[1 + kStatN];
    HIP_TRY(hipMemcpy(red, p->red, sizeof(red), hipMemcpyDeviceToHost));
    for (int k = 0; k < kStatN; k++) out7_host[k] = red[1 + k];
    out7_host[5] = sqrt(red[0]);
    out7_host[6] = (double)p->steps;
    return CRL_OK;
}

int crl_ppo_teacher_stats(crl_ppo *p, double *out4_host) {
    crl_fail_no_ctx();
    if (!p || !out4_host) return crl_fail(CRL_EINVAL, "crl_ppo_teacher_stats: null argument");
    if (!p->have_grad || !p->teacher_grad)
        return crl_fail(CRL_EINVAL, "crl_ppo_teacher_stats: the last gradient had no teacher (crl_ppo_grad_teacher)");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out4_host, p->red + 1 + kStatN, kStatT * sizeof(double), hipMemcpyDeviceToHost));
    return CRL_OK;
}

int crl_ppo_get_state(crl_ppo *p, float *blob_out_host, float *m_out_host, float *v_out_host, int64_t blob_floats, int64_t *steps_out,
                      int64_t *scratch_rows_out, void *stream) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_ppo_get_state: null learner");
    if ((blob_out_host || m_out_host || v_out_host) && blob_floats != p->blob_floats)
        return crl_fail(CRL_EINVAL, "crl_ppo_get_state: blob_floats %lld, but this learner's blob holds %d", (long long)blob_floats, p->blob_floats);
    if (int rc = ppo_read_state(p, blob_out_host, m_out_host, v_out_host, steps_out, (hipStream_t)stream)) return rc;
    if (scratch_rows_out) *scratch_rows_out = p->full ? ppo_full_scratch_rows(p->full) : 0;
    return CRL_OK;
}

int crl_ppo_set_state(crl_ppo *p, const float *blob_host, const float *m_host, const float *v_host, int64_t blob_floats, int64_t steps, void *stream) {
    crl_fail_no_ctx();
    if (!p || !blob_host || !m_host || !v_host) return crl_fail(CRL_EINVAL, "crl_ppo_set_state: null argument (weights and both moments are set together)");
    if (blob_floats != p->blob_floats)
        return crl_fail(CRL_EINVAL, "crl_ppo_set_state: blob_floats %lld, but this learner's blob holds %d", (long long)blob_floats, p->blob_floats);
    if (steps < 0) return crl_fail(CRL_EINVAL, "crl_ppo_set_state: steps must be >= 0, not %lld", (long long)steps);
    if (int rc = ppo_write_state(p, blob_host, m_host, v_host, steps, (hipStream_t)stream)) return rc;
    p->teacher_grad = false;
    return CRL_OK;
}

}  // extern "C"

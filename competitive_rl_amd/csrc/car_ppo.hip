// car_ppo.hip -- the CarRacing learner's PPO update on the device (include/crl.h "car ppo update"): the gradient of the clipped-surrogate
// loss of the car policy's MLP(21, 2) with its Gaussian head, straight from the sample lines of car_rollout.hip, and clip + Adam on the
// master weights, which ARE a car policy blob: crl_car_policy_set_weights takes the device pointer as it is.
//
// Gradient kernel.  One wavefront per workgroup; a workgroup takes groups of G = 64 consecutive idx entries: group w, w + W, ... of
// W = min(1024, ceil(B / 64)) workgroups -- a function of B alone.  Per group:
//   forward   a lane per sample: its line (eight dwordx4 loads), the hidden layer in float32 in the serving kernel's order (fc1_b, then
//             inputs 0..20), the three heads summed in float64 over the hidden units in order, then the loss terms and the three
//             derivative heads d mean_0, d mean_1, d v in closed form, float64, rounded once to float32.  x, relu(a) and the heads go to
//             LDS transposed ([feature][sample], [unit][sample], row stride 68: both the lane-per-sample stores and the operand loads
//             below are free of bank conflicts);
//   backward  on v_mfma_f32_16x16x4_f32 with the samples as the K dimension, four per instruction, 16 steps per group:
//             dW1^T[21 -> 32][100 -> 112] = sum_b x[b][k] da[b][j], da = relu'(a) ((d0 wp0_j + d1 wp1_j) + dv wv_j) formed by the lane
//             that feeds it, with row 21 of x held at 1 so that row 21 of the product is fc1_b's gradient: 14 accumulator tiles; and
//             the heads' weights, rows (d0, d1, dv) against relu(a): 7 more.  The tiles are summed over all the workgroup's groups.
//   biases    policy_b, value_b, log_std: per-lane float64 sums of the UNROUNDED closed forms over the lane's samples of all groups,
//             then the butterfly in float64: these five numbers are means of signed terms that cancel, and five float64 additions
//             per sample cost nothing beside the hidden layer.
// A workgroup writes its blob of partial sums; the reduce kernel adds them in workgroup order and divides by float32(max(L, 1)) (the
// five float64 sums: added in float64, divided by L in float64 and rounded once).
// No floating-point atomics: the same idx gives the same bits.
//
// Teacher targets ("car ppo update, teacher targets"): the <true> instantiation of the gradient kernel.  A lane loads one more 8-byte
// row (and 4 bytes of value target) with its line, the teacher term joins the closed forms of the two means and the two log_std in
// float64 in front of their one rounding, and four more per-lane float64 sums travel in rows of their own (tstat_part), so that the
// plain launch's rows, and its code, stay what they were.
#include <float.h>
#include <math.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "car_learner.h"
#include "ppo_optim.h"

#pragma clang fp contract(off)

namespace crl {

static constexpr int kHid = CRL_CAR_POLICY_HIDDEN, kFeat = CRL_CAR_OBS_FEATURES, kBlob = CRL_CAR_POLICY_BLOB_FLOATS;
static constexpr int kOffB1 = kFeat * kHid, kOffPol = kOffB1 + kHid, kOffVal = kOffPol + 2 * kHid, kOffTail = kOffVal + kHid;
static constexpr int kParams = kOffTail + 5;  // trained floats: everything in front of the two std floats and the pad
static_assert(kOffTail + 8 == kBlob && kParams == 2505, "blob layout of include/crl.h \"car policy\"");
static constexpr int kG = 64;        // samples per group: a lane each
static constexpr int kMaxW = 1024;   // workgroups at most
static constexpr int kStride = 68;   // row stride of the transposed LDS arrays
static constexpr int kHidPad = 112, kW1Row = 24;
static constexpr int kStat = 6;      // policy loss, value loss, entropy, old_logp - logp, clipped, live
static constexpr int kStatRow = kStat + 5;  // a workgroup's row of float64 sums: the statistics, then the five bias sums
static constexpr int kStatT = 4;     // a teacher gradient's own row: term, kl, abs_err, taught
static constexpr int kRedBlocks = (kBlob + 255) / 256;
#define CRL_LN_2PI_F64 1.8378770664093453

typedef float f4 __attribute__((ext_vector_type(4)));

struct CarPpoHyperDev {
    float clip, vf, ent;
};

struct CarGradArgs {
    CarRolloutView view;
    const int64_t *idx;
    int64_t count;
    const float *blob;
    float *partials;    // [W][kBlob]
    double *stat_part;  // [W][kStatRow]
    CarPpoHyperDev h;
};

// include/crl.h "car ppo update, teacher targets" as the teacher instantiation carries it
struct CarTeacherDev {
    const float2 *target;   // [T * R]: the teacher's action or mean
    const float *vtarget;   // [T * R] or null = the stored returns
    double *tstat_part;     // [W][kStatT]: the workgroups' teacher sums, a buffer of their own
    double sq0, sq1;        // exp(2 lsq_d); 0 for a point teacher
    double hq;              // (lsq_0 + lsq_1) + (1 + ln 2 pi): what kl takes off ce
    double coef;
    bool mse, kl, policy_term;
};

struct CarGradArgsTeacher : CarGradArgs {  // (built as CarGradArgsTeacher{a, t})
    CarTeacherDev t;
};

__device__ __forceinline__ double wave_sum_f64(double p) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_xor(p, m, 64);
    return p;
}

// kTeacher: include/crl.h "car ppo update, teacher targets" -- a lane also loads its sample's target row (and value target), the teacher
// term joins the closed forms in float64 before their one rounding, and four more statistics are summed.  <false> is what
// crl_car_ppo_grad launches.
template <bool kTeacher>
__global__ __launch_bounds__(64) void car_ppo_grad_kernel(std::conditional_t<kTeacher, CarGradArgsTeacher, CarGradArgs> a) {
    __shared__ __attribute__((aligned(16))) float sh_w1[kHid * kW1Row];  // fc1_w[j][k], rows padded to 24
    __shared__ float sh_b1[kHid], sh_wp0[kHidPad], sh_wp1[kHidPad], sh_wv[kHidPad];
    __shared__ float sh_h[kHidPad * kStride];  // relu(a)[j][sample]; rows 100..111 stay zero
    __shared__ float sh_x[32 * kStride];       // x[k][sample]; row 21 = live, rows 22..31 stay zero
    __shared__ float sh_d[3 * kG];             // d mean_0, d mean_1, d v per sample
    const int lane = threadIdx.x;
    const float *__restrict__ W = a.blob;
    for (int i = lane; i < kHid * kW1Row; i += 64) {
        const int j = i / kW1Row, k = i - j * kW1Row;
        sh_w1[i] = k < kFeat ? W[k * kHid + j] : 0.f;
    }
    for (int i = lane; i < kHidPad; i += 64) {
        const bool in = i < kHid;
        if (in) sh_b1[i] = W[kOffB1 + i];
        sh_wp0[i] = in ? W[kOffPol + i] : 0.f, sh_wp1[i] = in ? W[kOffPol + kHid + i] : 0.f, sh_wv[i] = in ? W[kOffVal + i] : 0.f;
    }
    for (int i = lane; i < kHidPad * kStride; i += 64) sh_h[i] = 0.f;
    for (int i = lane; i < 32 * kStride; i += 64) sh_x[i] = 0.f;
    const double bp0 = (double)W[kOffTail], bp1 = (double)W[kOffTail + 1], bv = (double)W[kOffTail + 2];
    const double ls0 = (double)W[kOffTail + 3], ls1 = (double)W[kOffTail + 4];
    const double sd0 = exp(ls0), sd1 = exp(ls1);
    __syncthreads();

    const int lj = lane & 15, lk = lane >> 4;
    float wp0r[7], wp1r[7], wvr[7];
#pragma unroll
    for (int jt = 0; jt < 7; jt++) wp0r[jt] = sh_wp0[jt * 16 + lj], wp1r[jt] = sh_wp1[jt * 16 + lj], wvr[jt] = sh_wv[jt * 16 + lj];
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f4 acc[3][7];
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int jt = 0; jt < 7; jt++) acc[m][jt] = zero4;
    double gb[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // policy_b[0], policy_b[1], value_b, log_std_0, log_std_1
    double st[kStat] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    [[maybe_unused]] double ts[kStatT] = {0.0, 0.0, 0.0, 0.0};

    const int64_t ngroups = (a.count + kG - 1) / kG;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b = g * kG + lane;
        const bool valid = b < a.count;
        // ---- forward: a lane per sample
        uint32_t flat = 0;
        if (valid) {
            const uint32_t raw = (uint32_t)a.idx[b];  // (a bad index only reads inside the array, as in the gather)
            flat = raw < a.view.last ? raw : a.view.last;
        }
        const float4 *__restrict__ src = reinterpret_cast<const float4 *>(a.view.lines + (int64_t)flat * kCarLineWords);
        float q[kCarLineWords];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float4 v = src[c];
            q[4 * c] = v.x, q[4 * c + 1] = v.y, q[4 * c + 2] = v.z, q[4 * c + 3] = v.w;
        }
        [[maybe_unused]] float2 tg = {0.f, 0.f};  // the teacher's row of sample idx[b] (an entry past count reads row 0 and is not live)
        [[maybe_unused]] float vt = 0.f;
        if constexpr (kTeacher) {
            tg = a.t.target[flat];
            if (a.t.vtarget) vt = a.t.vtarget[flat];
        }
        const bool live = valid && (__float_as_uint(q[kCarLineFlags]) & kCarFlagLive);
#pragma unroll
        for (int k = 0; k < kFeat; k++) {
            q[k] = valid ? q[k] : 0.f;
            sh_x[k * kStride + lane] = q[k];
        }
        sh_x[kFeat * kStride + lane] = live ? 1.f : 0.f;
        double m0 = 0.0, m1 = 0.0, vv = 0.0;
        for (int j = 0; j < kHid; j++) {
            const float4 *__restrict__ wr = reinterpret_cast<const float4 *>(sh_w1 + j * kW1Row);
            float wk[kW1Row];
#pragma unroll
            for (int c = 0; c < kW1Row / 4; c++) {
                const float4 v = wr[c];
                wk[4 * c] = v.x, wk[4 * c + 1] = v.y, wk[4 * c + 2] = v.z, wk[4 * c + 3] = v.w;
            }
            float pre = sh_b1[j];
#pragma unroll
            for (int k = 0; k < kFeat; k++) pre = pre + wk[k] * q[k];
            const float h = pre > 0.f ? pre : 0.f;
            sh_h[j * kStride + lane] = h;
            const double hd = (double)h;
            m0 = m0 + hd * (double)sh_wp0[j], m1 = m1 + hd * (double)sh_wp1[j], vv = vv + hd * (double)sh_wv[j];
        }
        float d0 = 0.f, d1 = 0.f, dv = 0.f;
        if (live) {
            const double mean0 = m0 + bp0, mean1 = m1 + bp1, v = vv + bv;
            const double olp = (double)q[kCarLineLogp], ret = (double)q[kCarLineReturn];
            const double A = (double)adv_out(q[kCarLineAdv], a.view.stats);
            const double zz0 = ((double)q[kCarLineU] - mean0) / sd0, zz1 = ((double)q[kCarLineU + 1] - mean1) / sd1;
            const double logp = ((-0.5 * (zz0 * zz0) - ls0) + (-0.5 * (zz1 * zz1) - ls1)) - CRL_LN_2PI_F64;
            const double ratio = exp(logp - olp);
            const double lo = 1.0 - (double)a.h.clip, hi = 1.0 + (double)a.h.clip;
            const double surr1 = ratio * A, surr2 = fmin(fmax(ratio, lo), hi) * A;
            const bool active = (A >= 0.0 && ratio < hi) || (A < 0.0 && ratio > lo);
            double glp = active ? -(A * ratio) : 0.0;
            if constexpr (kTeacher) glp = a.t.policy_term ? glp : 0.0;
            double dm0 = glp * zz0 / sd0, dm1 = glp * zz1 / sd1;
            double dl0 = glp * (zz0 * zz0 - 1.0) - (double)a.h.ent, dl1 = glp * (zz1 * zz1 - 1.0) - (double)a.h.ent;
            double target_v = ret;
            if constexpr (kTeacher) {
                if (a.t.vtarget) target_v = (double)vt;
                if (fabsf(tg.x) <= FLT_MAX && fabsf(tg.y) <= FLT_MAX) {  // taught: an untaught sample's term is 0 by selection
                    const double e0 = mean0 - (double)tg.x, e1 = mean1 - (double)tg.y;
                    double term, tm0 = e0, tm1 = e1, tl0 = 0.0, tl1 = 0.0;
                    if (a.t.mse) {
                        term = 0.5 * (e0 * e0 + e1 * e1);
                    } else {
                        const double var0 = sd0 * sd0, var1 = sd1 * sd1;
                        const double s0 = a.t.sq0 + e0 * e0, s1 = a.t.sq1 + e1 * e1;
                        term = ((ls0 + s0 / (2.0 * var0)) + (ls1 + s1 / (2.0 * var1))) + CRL_LN_2PI_F64;
                        tm0 = e0 / var0, tm1 = e1 / var1;
                        tl0 = 1.0 - s0 / var0, tl1 = 1.0 - s1 / var1;
                    }
                    dm0 = dm0 + a.t.coef * tm0, dm1 = dm1 + a.t.coef * tm1;  // (the teacher term is added last)
                    dl0 = dl0 + a.t.coef * tl0, dl1 = dl1 + a.t.coef * tl1;
                    ts[0] += term, ts[1] += a.t.kl ? term - a.t.hq : 0.0, ts[2] += (fabs(e0) + fabs(e1)) / 2.0, ts[3] += 1.0;
                }
            }
            const double dif = v - target_v;
            const double dvd = (double)a.h.vf * dif;
            d0 = (float)dm0, d1 = (float)dm1, dv = (float)dvd;
            gb[0] += dm0, gb[1] += dm1, gb[2] += dvd;
            gb[3] += dl0;
            gb[4] += dl1;
            st[0] += -fmin(surr1, surr2), st[1] += 0.5 * (dif * dif), st[2] += (ls0 + ls1) + (1.0 + CRL_LN_2PI_F64);
            st[3] += olp - logp, st[4] += (ratio < lo || ratio > hi) ? 1.0 : 0.0, st[5] += 1.0;
        }
        sh_d[lane] = d0, sh_d[kG + lane] = d1, sh_d[2 * kG + lane] = dv;
        __syncthreads();
        // ---- backward: the samples are the K dimension, four per instruction
        const int nvalid = (int)(a.count - g * kG < kG ? a.count - g * kG : kG);
        for (int s = 0; 4 * s < nvalid; s++) {
            const int bb = 4 * s + lk;
            const float e0 = sh_d[bb], e1 = sh_d[kG + bb], ev = sh_d[2 * kG + bb];
            const float x0 = sh_x[lj * kStride + bb], x1 = sh_x[(16 + lj) * kStride + bb];
            const float hd = lj == 0 ? e0 : lj == 1 ? e1 : lj == 2 ? ev : 0.f;
#pragma unroll
            for (int jt = 0; jt < 7; jt++) {
                const float h = sh_h[(jt * 16 + lj) * kStride + bb];
                const float da = h > 0.f ? (e0 * wp0r[jt] + e1 * wp1r[jt]) + ev * wvr[jt] : 0.f;
                acc[0][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, da, acc[0][jt], 0, 0, 0);
                acc[1][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, da, acc[1][jt], 0, 0, 0);
                acc[2][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(hd, h, acc[2][jt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- the workgroup's partial blob.  D: rows 4 lk + r, columns lj
    float *__restrict__ P = a.partials + (int64_t)blockIdx.x * kBlob;
#pragma unroll
    for (int jt = 0; jt < 7; jt++) {
        const int j = jt * 16 + lj;
        if (j >= kHid) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int k0 = 4 * lk + r, k1 = 16 + k0;
            P[k0 * kHid + j] = acc[0][jt][r];
            if (k1 < kFeat) P[k1 * kHid + j] = acc[1][jt][r];
            else if (k1 == kFeat) P[kOffB1 + j] = acc[1][jt][r];
            if (k0 < 3) P[kOffPol + k0 * kHid + j] = acc[2][jt][r];  // policy_w[0], policy_w[1], value_w
        }
    }
    if (lane < 8) P[kOffTail + lane] = 0.f;  // the five bias sums travel in float64; the std floats and the pad are not trained
#pragma unroll
    for (int k = 0; k < kStat; k++) {
        const double sum = wave_sum_f64(st[k]);
        if (lane == 0) a.stat_part[(int64_t)blockIdx.x * kStatRow + k] = sum;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const double sum = wave_sum_f64(gb[k]);
        if (lane == 0) a.stat_part[(int64_t)blockIdx.x * kStatRow + kStat + k] = sum;
    }
    if constexpr (kTeacher) {
#pragma unroll
        for (int k = 0; k < kStatT; k++) {
            const double sum = wave_sum_f64(ts[k]);
            if (lane == 0) a.t.tstat_part[(int64_t)blockIdx.x * kStatT + k] = sum;
        }
    }
}

// x[0] + x[stride] + .. + x[(count - 1) stride], added in this order; the loads go out kBurst at a time (the sum of up to 1024 partials
// is a chain of additions, but nothing makes its loads wait for one another)
static constexpr int kBurst = 16;
template <class T>
__device__ __forceinline__ T ordered_sum(const T *__restrict__ x, int count, int64_t stride) {
    T sum = (T)0;
    int w = 0;
    for (; w + kBurst <= count; w += kBurst) {
        T v[kBurst];
#pragma unroll
        for (int k = 0; k < kBurst; k++) v[k] = x[(int64_t)(w + k) * stride];
#pragma unroll
        for (int k = 0; k < kBurst; k++) sum += v[k];
    }
    for (; w < count; w++) sum += x[(int64_t)w * stride];
    return sum;
}

// red[1 .. 5] = the statistics' means over the live samples, red[6] = L: lane s adds the workgroups' sums in workgroup order
// kTeacher: lanes 6 .. 9 fold the teacher rows the same way into tred[0 .. 3]: the means of term, kl and abs_err over the Lt taught
// samples, and Lt / max(L, 1)
template <bool kTeacher>
__global__ __launch_bounds__(64) void car_ppo_stats_kernel(const double *__restrict__ stat_part, int groups, double *__restrict__ red,
                                                           const double *__restrict__ tstat_part, double *__restrict__ tred) {
    const int s = threadIdx.x;
    if constexpr (kTeacher) {
        if (s >= kStat && s < kStat + kStatT) {
            const int k = s - kStat;
            const double taught = ordered_sum(tstat_part + kStatT - 1, groups, kStatT);
            if (k == kStatT - 1) {
                const double live = ordered_sum(stat_part + kStat - 1, groups, kStatRow);
                tred[k] = taught / (live > 1.0 ? live : 1.0);
            } else {
                tred[k] = ordered_sum(tstat_part + k, groups, kStatT) / (taught > 1.0 ? taught : 1.0);
            }
        }
    }
    if (s >= kStat) return;
    const double live = ordered_sum(stat_part + kStat - 1, groups, kStatRow), sum = ordered_sum(stat_part + s, groups, kStatRow);
    red[1 + s] = s == kStat - 1 ? live : sum / (live > 1.0 ? live : 1.0);
}

// pong_ppo.h's ppo_reduce_kernel with the divisor read on the device: float32(max(L, 1))
__global__ __launch_bounds__(256) void car_ppo_reduce_kernel(const float *__restrict__ partials, const double *__restrict__ stat_part, int groups,
                                                            const double *__restrict__ red, float *__restrict__ grad, double *__restrict__ sq_part) {
    __shared__ double s[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double L = red[kStat];
    const float count_f = (float)(L > 1.0 ? L : 1.0);
    float g = 0.f;
    if (i >= kOffTail && i < kParams) {  // policy_b, value_b, log_std: the float64 sums, rounded once
        const int k = kStat + (i - kOffTail);
        const double sum = ordered_sum(stat_part + k, groups, kStatRow);
        g = (float)(sum / (L > 1.0 ? L : 1.0));
        grad[i] = g;
    } else if (i < kBlob) {
        const float sum = ordered_sum(partials + i, groups, kBlob);
        g = sum / count_f;
        grad[i] = g;
    }
    s[threadIdx.x] = (double)g * (double)g;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq_part[blockIdx.x] = s[0];
}

struct CarStepArgs {
    AdamBlobs b;
    const double *sq_part;
    AdamArgs h;
};

// include/crl.h "ppo update", optimiser step, unchanged, over the 2505 trained floats; the lane of log_std_d then rewrites std_d
__global__ __launch_bounds__(256) void car_ppo_step_kernel(CarStepArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kParams) return;
    double sq = a.sq_part[0];
    for (int k = 1; k < kRedBlocks; k++) sq += a.sq_part[k];
    const float p = adam_lane(a.h, a.b, i, sq);
    a.b.raw[i] = p;
    if (i >= kOffTail + 3) a.b.raw[i + 2] = (float)exp((double)p);  // the serving kernel evaluates no exp
}

}  // namespace crl

using namespace crl;

struct crl_car_ppo : PpoBlobs {  // blob_floats is kBlob
    float *partials = nullptr;
    double *stat_part = nullptr, *sq_part = nullptr, *red = nullptr;  // red[1 .. 5]: the statistics' means, red[6]: L
    double *tstat_part = nullptr, *tred = nullptr;                    // a teacher gradient's rows [kMaxW][kStatT] and its four statistics
    bool teacher_grad = false;                                        // the last gradient was crl_car_ppo_grad_teacher's
};

extern "C" {

void crl_car_ppo_destroy(crl_car_ppo *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    ppo_free_blobs(p);
    for (void *q : {(void *)p->partials, (void *)p->stat_part, (void *)p->sq_part, (void *)p->red, (void *)p->tstat_part, (void *)p->tred})
        if (q) (void)hipFree(q);
    delete p;
}

int crl_car_ppo_set_weights(crl_car_ppo *p, const float *blob_host) {
    crl_fail_no_ctx();
    if (!p || !blob_host) return crl_fail(CRL_EINVAL, "crl_car_ppo_set_weights: null argument");
    std::vector<float> blob(blob_host, blob_host + kBlob);
    for (int i = 0; i < kParams; i++)
        if (!(fabsf(blob[i]) <= FLT_MAX)) return crl_fail(CRL_EINVAL, "crl_car_ppo_set_weights: float %d of the blob is not finite", i);
    for (int d = 0; d < 2; d++) blob[kOffTail + 5 + d] = (float)exp((double)blob[kOffTail + 3 + d]);  // derived, not trained
    blob[kBlob - 1] = 0.f;
    return ppo_upload(p, blob.data());
}

int crl_car_ppo_create(int32_t device, const float *blob_host, crl_car_ppo **out) {
    crl_fail_no_ctx();
    if (!out || !blob_host) return crl_fail(CRL_EINVAL, "crl_car_ppo_create: null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    crl_car_ppo *p = new crl_car_ppo();
    p->device = device;
    const char *who = "crl_car_ppo_create";
    int rc = ppo_alloc_blobs(p, kBlob, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->partials, (size_t)kMaxW * kBlob * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->stat_part, (size_t)kMaxW * kStatRow * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->sq_part, kRedBlocks * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->red, (1 + kStat) * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->tstat_part, (size_t)kMaxW * kStatT * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->tred, kStatT * sizeof(double), who);
    if (rc == CRL_OK) rc = crl_car_ppo_set_weights(p, blob_host);
    if (rc != CRL_OK) {
        crl_car_ppo_destroy(p);
        return rc;
    }
    *out = p;
    return CRL_OK;
}

int crl_car_ppo_get_weights(crl_car_ppo *p, float *blob_out_host) {
    crl_fail_no_ctx();
    if (!p || !blob_out_host) return crl_fail(CRL_EINVAL, "crl_car_ppo_get_weights: null argument");
    return ppo_download(p, blob_out_host);
}

int crl_car_ppo_weights_dev(crl_car_ppo *p, const float **blob_dev) {
    crl_fail_no_ctx();
    if (!p || !blob_dev) return crl_fail(CRL_EINVAL, "crl_car_ppo_weights_dev: null argument");
    *blob_dev = p->raw;
    return CRL_OK;
}

}  // extern "C"

// the three launches; kTeacher chooses the instantiations
template <bool kTeacher>
static void car_ppo_launch(crl_car_ppo *p, const std::conditional_t<kTeacher, CarGradArgsTeacher, CarGradArgs> &a, int groups, hipStream_t st) {
    hipLaunchKernelGGL(car_ppo_grad_kernel<kTeacher>, dim3(groups), dim3(64), 0, st, a);
    hipLaunchKernelGGL(car_ppo_stats_kernel<kTeacher>, dim3(1), dim3(64), 0, st, p->stat_part, groups, p->red, p->tstat_part, p->tred);
    hipLaunchKernelGGL(car_ppo_reduce_kernel, dim3(kRedBlocks), dim3(256), 0, st, p->partials, p->stat_part, groups, p->red, p->grad, p->sq_part);
}

// crl_car_ppo_grad (teacher null) and crl_car_ppo_grad_teacher: everything is looked at before the learner or the GPU is touched
static int car_ppo_grad(const char *who, crl_car_ppo *p, const crl_car_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper,
                        const crl_car_ppo_teacher *teacher, void *stream) {
    if (!p || !rollout || !idx_dev) return crl_fail(CRL_EINVAL, "%s: null argument", who);
    if ((uintptr_t)idx_dev & 7) return crl_fail(CRL_EINVAL, "%s: idx must be 8-byte aligned", who);
    if (count < 1 || count > 0x7fffffff) return crl_fail(CRL_EINVAL, "%s: the number of samples must be in [1, 2^31)", who);
    if (int rc = ppo_hyper_check(who, hyper)) return rc;
    const CarRolloutView view = car_rollout_view(rollout);
    if (!view.finished) return crl_fail(CRL_EINVAL, "%s: the rollout is not finished (crl_car_rollout_finish computes returns and advantages)", who);
    CarTeacherDev t{};
    if (teacher) {
        if (!teacher->target_dev) return crl_fail(CRL_EINVAL, "%s: the teacher has no target", who);
        if (teacher->rows != (int64_t)view.last + 1)
            return crl_fail(CRL_EINVAL, "%s: the teacher holds %lld rows, the rollout's T * R is %lld", who, (long long)teacher->rows, (long long)view.last + 1);
        if (teacher->kind != CRL_CAR_TEACHER_CE && teacher->kind != CRL_CAR_TEACHER_MSE)
            return crl_fail(CRL_EINVAL, "%s: kind must be CRL_CAR_TEACHER_CE or CRL_CAR_TEACHER_MSE, not %d", who, (int)teacher->kind);
        if (teacher->point != 0 && teacher->point != 1) return crl_fail(CRL_EINVAL, "%s: point must be 0 or 1, not %d", who, (int)teacher->point);
        if (teacher->policy_term != 0 && teacher->policy_term != 1)
            return crl_fail(CRL_EINVAL, "%s: policy_term must be 0 or 1, not %d", who, (int)teacher->policy_term);
        if (!(teacher->coef >= 0.f && teacher->coef <= FLT_MAX)) return crl_fail(CRL_EINVAL, "%s: coef must be finite and >= 0", who);
        if (!teacher->point && !(fabsf(teacher->teacher_log_std[0]) <= FLT_MAX && fabsf(teacher->teacher_log_std[1]) <= FLT_MAX))
            return crl_fail(CRL_EINVAL, "%s: teacher_log_std must be finite (point = 1 is the teacher without a spread)", who);
        if (((uintptr_t)teacher->target_dev & 7) || ((uintptr_t)teacher->value_targets_dev & 3))
            return crl_fail(CRL_EINVAL, "%s: the target must be 8-byte aligned, the value targets 4-byte aligned", who);
        const double lsq0 = teacher->point ? 0.0 : (double)teacher->teacher_log_std[0], lsq1 = teacher->point ? 0.0 : (double)teacher->teacher_log_std[1];
        t.target = reinterpret_cast<const float2 *>(teacher->target_dev), t.vtarget = teacher->value_targets_dev, t.tstat_part = p->tstat_part;
        t.sq0 = teacher->point ? 0.0 : exp(2.0 * lsq0), t.sq1 = teacher->point ? 0.0 : exp(2.0 * lsq1);
        t.hq = (lsq0 + lsq1) + (1.0 + CRL_LN_2PI_F64);
        t.coef = (double)teacher->coef, t.mse = teacher->kind == CRL_CAR_TEACHER_MSE, t.kl = !t.mse && !teacher->point, t.policy_term = teacher->policy_term != 0;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t ngroups = (count + kG - 1) / kG;
    const int groups = (int)(ngroups < kMaxW ? ngroups : kMaxW);
    const CarGradArgs a{view, idx_dev, count, p->raw, p->partials, p->stat_part, CarPpoHyperDev{hyper->clip, hyper->vf_coef, hyper->ent_coef}};
    if (teacher) car_ppo_launch<true>(p, CarGradArgsTeacher{a, t}, groups, st);
    else car_ppo_launch<false>(p, a, groups, st);
    HIP_TRY(hipGetLastError());
    p->have_grad = true, p->teacher_grad = teacher != nullptr;
    return CRL_OK;
}

extern "C" {

int crl_car_ppo_grad(crl_car_ppo *p, const crl_car_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper, void *stream) {
    crl_fail_no_ctx();
    return car_ppo_grad("crl_car_ppo_grad", p, rollout, idx_dev, count, hyper, nullptr, stream);
}

int crl_car_ppo_grad_teacher(crl_car_ppo *p, const crl_car_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper,
                             const crl_car_ppo_teacher *teacher, void *stream) {
    crl_fail_no_ctx();
    if (!teacher) return crl_fail(CRL_EINVAL, "crl_car_ppo_grad_teacher: null teacher (crl_car_ppo_grad is the plain gradient)");
    return car_ppo_grad("crl_car_ppo_grad_teacher", p, rollout, idx_dev, count, hyper, teacher, stream);
}

int crl_car_ppo_teacher_stats(crl_car_ppo *p, double *out4_host) {
    crl_fail_no_ctx();
    if (!p || !out4_host) return crl_fail(CRL_EINVAL, "crl_car_ppo_teacher_stats: null argument");
    if (!p->have_grad || !p->teacher_grad)
        return crl_fail(CRL_EINVAL, "crl_car_ppo_teacher_stats: the last gradient had no teacher (crl_car_ppo_grad_teacher)");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out4_host, p->tred, kStatT * sizeof(double), hipMemcpyDeviceToHost));
    return CRL_OK;
}

int crl_car_ppo_get_grad(crl_car_ppo *p, const float **grad_dev, float *grad_out_host) {
    crl_fail_no_ctx();
    if (!p || (!grad_dev && !grad_out_host)) return crl_fail(CRL_EINVAL, "crl_car_ppo_get_grad: null argument");
    if (!p->have_grad) return crl_fail(CRL_EINVAL, "crl_car_ppo_get_grad: no gradient yet (crl_car_ppo_grad)");
    return ppo_read_grad(p, grad_dev, grad_out_host);
}

int crl_car_ppo_step(crl_car_ppo *p, const crl_ppo_hyper *hyper, void *stream) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_car_ppo_step: null learner");
    if (int rc = ppo_hyper_check("crl_car_ppo_step", hyper)) return rc;
    if (!p->have_grad) return crl_fail(CRL_EINVAL, "crl_car_ppo_step: no gradient yet (crl_car_ppo_grad)");
    const int64_t t = p->steps + 1;
    const CarStepArgs a{p->adam(), p->sq_part, adam_args(hyper, t)};
    hipLaunchKernelGGL(car_ppo_step_kernel, dim3((kParams + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    p->steps = t;
    return CRL_OK;
}

int crl_car_ppo_stats(crl_car_ppo *p, double *out8_host) {
    crl_fail_no_ctx();
    if (!p || !out8_host) return crl_fail(CRL_EINVAL, "crl_car_ppo_stats: null argument");
    if (!p->have_grad) return crl_fail(CRL_EINVAL, "crl_car_ppo_stats: no gradient yet (crl_car_ppo_grad)");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    double red[1 + kStat], sq[kRedBlocks];
    HIP_TRY(hipMemcpy(red, p->red, sizeof(red), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sq, p->sq_part, sizeof(sq), hipMemcpyDeviceToHost));
    double sum = sq[0];
    for (int k = 1; k < kRedBlocks; k++) sum += sq[k];  // (the step kernel's order)
    for (int k = 0; k < 5; k++) out8_host[k] = red[1 + k];
    out8_host[5] = sqrt(sum);
    out8_host[6] = (double)p->steps;
    out8_host[7] = red[kStat];
    return CRL_OK;
}

int crl_car_ppo_get_state(crl_car_ppo *p, float *blob_out_host, float *m_out_host, float *v_out_host, int64_t *steps_out, void *stream) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_car_ppo_get_state: null learner");
    return ppo_read_state(p, blob_out_host, m_out_host, v_out_host, steps_out, (hipStream_t)stream);
}

int crl_car_ppo_set_state(crl_car_ppo *p, const float *blob_host, const float *m_host, const float *v_host, int64_t steps, void *stream) {
    crl_fail_no_ctx();
    if (!p || !blob_host || !m_host || !v_host) return crl_fail(CRL_EINVAL, "crl_car_ppo_set_state: null argument (weights and both moments are set together)");
    if (steps < 0) return crl_fail(CRL_EINVAL, "crl_car_ppo_set_state: steps must be >= 0, not %lld", (long long)steps);
    return ppo_write_state(p, blob_host, m_host, v_host, steps, (hipStream_t)stream);
}

}  // extern "C"

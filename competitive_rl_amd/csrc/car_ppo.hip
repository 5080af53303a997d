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
#include <float.h>
#include <math.h>
#include <string.h>

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

__device__ __forceinline__ double wave_sum_f64(double p) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_xor(p, m, 64);
    return p;
}

__global__ __launch_bounds__(64) void car_ppo_grad_kernel(CarGradArgs a) {
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
            const double glp = active ? -(A * ratio) : 0.0;
            const double dm0 = glp * zz0 / sd0, dm1 = glp * zz1 / sd1;
            const double dif = v - ret;
            const double dvd = (double)a.h.vf * dif;
            d0 = (float)dm0, d1 = (float)dm1, dv = (float)dvd;
            gb[0] += dm0, gb[1] += dm1, gb[2] += dvd;
            gb[3] += glp * (zz0 * zz0 - 1.0) - (double)a.h.ent;
            gb[4] += glp * (zz1 * zz1 - 1.0) - (double)a.h.ent;
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
__global__ __launch_bounds__(64) void car_ppo_stats_kernel(const double *__restrict__ stat_part, int groups, double *__restrict__ red) {
    const int s = threadIdx.x;
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
};

extern "C" {

void crl_car_ppo_destroy(crl_car_ppo *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    ppo_free_blobs(p);
    for (void *q : {(void *)p->partials, (void *)p->stat_part, (void *)p->sq_part, (void *)p->red})
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

int crl_car_ppo_grad(crl_car_ppo *p, const crl_car_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper, void *stream) {
    crl_fail_no_ctx();
    const char *who = "crl_car_ppo_grad";
    if (!p || !rollout || !idx_dev) return crl_fail(CRL_EINVAL, "%s: null argument", who);
    if ((uintptr_t)idx_dev & 7) return crl_fail(CRL_EINVAL, "%s: idx must be 8-byte aligned", who);
    if (count < 1 || count > 0x7fffffff) return crl_fail(CRL_EINVAL, "%s: the number of samples must be in [1, 2^31)", who);
    if (int rc = ppo_hyper_check(who, hyper)) return rc;
    const CarRolloutView view = car_rollout_view(rollout);
    if (!view.finished) return crl_fail(CRL_EINVAL, "%s: the rollout is not finished (crl_car_rollout_finish computes returns and advantages)", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t ngroups = (count + kG - 1) / kG;
    const int groups = (int)(ngroups < kMaxW ? ngroups : kMaxW);
    const CarGradArgs a{view, idx_dev, count, p->raw, p->partials, p->stat_part, CarPpoHyperDev{hyper->clip, hyper->vf_coef, hyper->ent_coef}};
    hipLaunchKernelGGL(car_ppo_grad_kernel, dim3(groups), dim3(64), 0, st, a);
    hipLaunchKernelGGL(car_ppo_stats_kernel, dim3(1), dim3(64), 0, st, p->stat_part, groups, p->red);
    hipLaunchKernelGGL(car_ppo_reduce_kernel, dim3(kRedBlocks), dim3(256), 0, st, p->partials, p->stat_part, groups, p->red, p->grad, p->sq_part);
    HIP_TRY(hipGetLastError());
    p->have_grad = true;
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

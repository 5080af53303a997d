// pong_rollout.hip -- a learner's rollout storage on the device (include/crl.h "rollout storage"): T steps of what crl_policy_act_rollout
// saw and wrote, kept as ONE new 42 x 42 plane per env and step -- the other three planes of a step's stack are the planes of the three
// steps before it, exactly as in the frame ring of pong_ring.h --, returns and advantages by GAE, and the gather that rebuilds the
// float32 (or uint8) stacks of a shuffled minibatch from four stored planes and the step's depth.
//
// Stands in for the rollout storage a trainer around the reference keeps on the host side of its loop (a float32 FrameStackTensor copy
// per step, utils/utils.py:145-173): 28 224 bytes per env and step there, 1 776 + 27 here.  An object of its own: nothing here reaches
// into a crl_policy, the caller passes the act call's inputs and outputs in.
#include <string.h>
#include "pong_ring.h"
#include "pong_rollout.h"
#include "rollout_core.h"

namespace crl {

static constexpr int kHist = CRL_POLICY_STACK - 1;  // rows 0..2 of `planes`: the three frames before step 0, oldest first

// crl_rollout_begin with a stack: planes 1..3 of u8 [n][4][42][42] -> rows 0..2 (a lane per dword; the 12 bytes of padding stay zero)
__global__ __launch_bounds__(256) void rollout_history_kernel(uint32_t *__restrict__ planes, const uint32_t *__restrict__ stack, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * kHist * kPlaneWords) return;
    const int64_t env = i / (kHist * kPlaneWords);
    const int r = (int)(i - env * (kHist * kPlaneWords));
    const int j = r / kPlaneWords, d = r - j * kPlaneWords;
    planes[((int64_t)j * n + env) * (kPlanePad / 4) + d] = stack[(env * CRL_POLICY_STACK + j + 1) * kPlaneWords + d];
}

// crl_rollout_begin without one: the depth that the finished rollout's last step hands on, min(3, depth[T-1])
__global__ __launch_bounds__(256) void rollout_carry_depth_kernel(const uint8_t *__restrict__ last_depth, uint8_t *__restrict__ carry, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) carry[e] = last_depth[e] < kHist ? last_depth[e] : (uint8_t)kHist;
}

struct RecordArgs {
    const uint8_t *frame;  // env e at frame + e * frame_stride, 4-byte aligned
    int64_t frame_stride;
    const uint8_t *reset;  // [n] or null
    const int32_t *actions;  // env e at actions[e * action_stride], or null
    int64_t action_stride;
    const float *values, *logp;  // [n] or null
    const uint8_t *depth_prev;   // [n]: depth[t-1], or the carry at t = 0
    uint32_t *row;               // planes row t + 3
    uint8_t *reset_out, *depth_out;
    int32_t *actions_out;
    float *values_out, *logp_out;
    int64_t n;
};

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // 16 bytes at a 4-byte aligned address: one dwordx4 load

// One launch per step: a lane per 16-byte chunk of the n padded planes (111 per env: the row is one contiguous run of uint4 stores; a
// frame is only 4-byte aligned, its chunk is read as one dwordx4 at that alignment; chunk 110 holds the last dword and the zero
// padding), and the first n lanes also write their env's scalars and its depth by the stack rule.
__global__ __launch_bounds__(256) void rollout_record_kernel(RecordArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) {
        const uint8_t rs = a.reset ? (uint8_t)(a.reset[i] != 0) : (uint8_t)0;
        const uint8_t dp = a.depth_prev[i];
        a.reset_out[i] = rs;
        a.depth_out[i] = rs ? (uint8_t)1 : (uint8_t)(dp + 1 < CRL_POLICY_STACK ? dp + 1 : CRL_POLICY_STACK);
        a.actions_out[i] = a.actions ? a.actions[i * a.action_stride] : 0;
        a.values_out[i] = a.values ? a.values[i] : 0.0f;
        a.logp_out[i] = a.logp ? a.logp[i] : 0.0f;
    }
    if (i >= a.n * kPlaneChunks) return;
    const int64_t env = i / kPlaneChunks;
    const int c = (int)(i - env * kPlaneChunks);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.frame + env * a.frame_stride) + c * 4;
    uint4 v{0u, 0u, 0u, 0u};
    if (c < kPlaneChunks - 1) {
        const u32x4_a4 w = *reinterpret_cast<const u32x4_a4 *>(src);
        v = uint4{w.x, w.y, w.z, w.w};
    } else {
        v.x = src[0];  // dword 440 of 441
    }
    reinterpret_cast<uint4 *>(a.row)[env * kPlaneChunks + c] = v;
}

__global__ __launch_bounds__(256) void rollout_outcome_kernel(const float *__restrict__ rewards, int64_t reward_stride, const uint8_t *__restrict__ done,
                                                             float *__restrict__ rewards_out, uint8_t *__restrict__ done_out, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    rewards_out[e] = rewards[e * reward_stride];
    done_out[e] = (uint8_t)(done[e] != 0);
}

// include/crl.h "GAE rule" (rollout_core.h): a lane per env walks t = T-1 .. 0 over the arrays
__global__ __launch_bounds__(256) void rollout_gae_kernel(const float *__restrict__ rewards, const float *__restrict__ values, const uint8_t *__restrict__ done,
                                                         const float *__restrict__ last_values, float g, float gl, float *__restrict__ adv,
                                                         float *__restrict__ ret, int64_t n, int steps) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float acc = 0.0f;
    float vnext = last_values ? last_values[e] : 0.0f;
    for (int t = steps - 1; t >= 0; t--) {
        const int64_t k = (int64_t)t * n + e;
        const bool d = done[k] != 0;  // (the loads in the order they always had: done, value, reward)
        const float v = values[k];
        gae_step(rewards[k], v, d, g, gl, acc, vnext, adv[k], ret[k]);
    }
}

struct PongAdvSrc {  // the statistics' source (rollout_core.h): every one of the T * n advantages takes part
    static constexpr bool kCounted = false;
    const float *__restrict__ x;
    __device__ bool live(int64_t) const { return true; }
    __device__ float adv(int64_t i) const { return x[i]; }
};

struct GatherArgs {
    const uint32_t *planes;  // [T + 3][n][kPlanePad / 4]
    const uint8_t *depth;    // [T * n]
    const int64_t *idx;      // [B]: t * n + e
    int64_t count;
    uint32_t n, last;  // last = T * n - 1
    void *obs;  // [B][4][42][42] float32 or uint8, or null
    const int32_t *actions;
    const float *logp, *values, *ret, *adv;
    int32_t *actions_out;
    float *logp_out, *values_out, *ret_out, *adv_out;  // each [B] or null
    const double *stats;                               // mean, std: read when the advantages are normalised, else null
};

// The hot path: a wavefront per sample.  The sample's flat index is wave-uniform, so its step, env and depth live in scalar registers;
// a lane reads one dword (four pixels) of a stored plane -- 7 x 64 lanes cover a plane's 441 dwords -- and stores one float4 (F32) or the
// dword as it is: 1 KiB resp. 256 contiguous bytes per wave-instruction, every output plane 16-byte resp. 4-byte aligned.  All loads of
// the sample's live planes are issued before the first store; a masked plane is zeros without a load.  Streaming: no LDS.
template <bool F32>
__global__ __launch_bounds__(256) void rollout_gather_kernel(GatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.count) return;
    // (T * n < 2^31: crl_rollout_create.  The indices' validity is the caller's; the clamp only keeps a bad one's READS inside the arrays)
    const uint32_t raw = __builtin_amdgcn_readfirstlane((uint32_t)a.idx[b]);
    const uint32_t flat = raw < a.last ? raw : a.last;
    const uint32_t t = flat / a.n, e = flat - t * a.n;
    if (a.obs) {
        const int dep = a.depth[flat];
        constexpr int kIter = (kPlaneWords + 63) / 64;  // 7
        uint32_t w[CRL_POLICY_STACK][kIter];
#pragma unroll
        for (int j = 0; j < CRL_POLICY_STACK; j++) {
            const uint32_t *src = a.planes + ((int64_t)(t + j) * a.n + e) * (kPlanePad / 4);
            const bool live = CRL_POLICY_STACK - 1 - j < dep;  // (wave-uniform)
#pragma unroll
            for (int q = 0; q < kIter; q++) {
                const int d = q * 64 + lane;
                w[j][q] = (live && d < kPlaneWords) ? src[d] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < CRL_POLICY_STACK; j++) {
#pragma unroll
            for (int q = 0; q < kIter; q++) {
                const int d = q * 64 + lane;
                if (d >= kPlaneWords) continue;
                const uint32_t v = w[j][q];
                const int64_t o = (b * CRL_POLICY_STACK + j) * kPlaneWords + d;
                if (F32) reinterpret_cast<float4 *>(a.obs)[o] = float4{(float)(v & 255u), (float)((v >> 8) & 255u), (float)((v >> 16) & 255u), (float)(v >> 24)};
                else reinterpret_cast<uint32_t *>(a.obs)[o] = v;
            }
        }
    }
    if (lane == 0) {
        if (a.actions_out) a.actions_out[b] = a.actions[flat];
        if (a.logp_out) a.logp_out[b] = a.logp[flat];
        if (a.values_out) a.values_out[b] = a.values[flat];
        if (a.ret_out) a.ret_out[b] = a.ret[flat];
        if (a.adv_out) a.adv_out[b] = adv_out(a.adv[flat], a.stats);
    }
}

}  // namespace crl

using namespace crl;

struct crl_rollout : RolloutSteps {
    int device = 0;
    int64_t n = 0;
    uint8_t *planes = nullptr, *reset = nullptr, *depth = nullptr, *depth_carry = nullptr, *done = nullptr;
    int32_t *actions = nullptr;
    float *logp = nullptr, *values = nullptr, *rewards = nullptr, *adv = nullptr, *ret = nullptr;
    double *stats = nullptr;  // mean, std, then kRedGroups partial sums
};

namespace crl {

// ---- rollout_core.h, the step counters' refusals, for both storages.  A text that names a sibling call forms it from who's prefix
static int family(const char *who) { return (int)(strrchr(who, '_') - who) + 1; }  // the length of crl_<storage>_

int RolloutSteps::check_record(const char *who, int64_t t) const {
    if (state == kFinished) return crl_fail(CRL_EINVAL, "%s: the rollout is finished; %.*sbegin starts the next one", who, family(who), who);
    if (t != recorded || t >= steps) return crl_fail(CRL_EINVAL, "%s: step %lld is not the next step (%d of %d steps recorded)", who, (long long)t, recorded, steps);
    return CRL_OK;
}

int RolloutSteps::check_outcome(const char *who, int64_t t) const {
    if (state == kActive && t == outcomes && t < recorded) return CRL_OK;
    return crl_fail(CRL_EINVAL, "%s: step %lld has no record, or has its outcome (%d steps recorded, %d outcomes)", who, (long long)t,
                    state == kActive ? recorded : 0, state == kActive ? outcomes : 0);
}

int RolloutSteps::check_finish(const char *who) const {
    return state != kFresh && outcomes == steps ? CRL_OK : crl_fail(CRL_EINVAL, "%s: %d of %d steps have their outcome", who, state == kFresh ? 0 : outcomes, steps);
}

int RolloutSteps::check_finished(const char *who) const {
    return state == kFinished ? CRL_OK : crl_fail(CRL_EINVAL, "%s: the rollout is not finished (%.*sfinish computes what a sample holds)", who, family(who), who);
}

int RolloutSteps::check_restore(const char *who, const int32_t *info4) const {
    const int st = info4[0], rec = info4[1], out = info4[2];
    if (st >= kFresh && st <= kFinished && out >= 0 && out <= rec && rec <= steps && (st != kFresh || rec == 0) && (st != kFinished || out == steps)) return CRL_OK;
    return crl_fail(CRL_EINVAL, "%s: state %d with %d steps recorded and %d outcomes does not fit a storage of %d steps", who, st, rec, out, steps);
}

void RolloutSteps::info(int32_t *out4) const {
    out4[0] = state, out4[1] = recorded, out4[2] = outcomes, out4[3] = normalize ? 1 : 0;
    if (state == kFinished) out4[1] = out4[2] = steps;
    if (state == kFresh) out4[1] = out4[2] = 0;
}

RolloutView rollout_view(const crl_rollout *r) {
    return RolloutView{r->planes, r->depth, r->actions, r->logp, r->ret, r->adv, r->normalize ? r->stats : nullptr, (uint32_t)r->n,
                       (uint32_t)(r->n * r->steps - 1), r->state == kFinished};
}
}  // namespace crl

extern "C" {

void crl_rollout_destroy(crl_rollout *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    for (void *p : {(void *)r->planes, (void *)r->reset, (void *)r->depth, (void *)r->depth_carry, (void *)r->done, (void *)r->actions, (void *)r->logp,
                    (void *)r->values, (void *)r->rewards, (void *)r->adv, (void *)r->ret, (void *)r->stats})
        if (p) (void)hipFree(p);
    delete r;
}

int crl_rollout_create(int32_t device, int64_t num_envs, int64_t num_steps, crl_rollout **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || num_steps <= 0 || num_envs > 0x7fffffff || num_steps > 0x7fffffff || num_envs * num_steps > 0x7fffffff)
        return crl_fail(CRL_EINVAL, "crl_rollout_create: bad arguments (num_envs >= 1, num_steps >= 1, num_envs * num_steps < 2^31)");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    crl_rollout *r = new crl_rollout();
    r->device = device, r->n = num_envs, r->steps = (int)num_steps;
    const size_t tn = (size_t)num_envs * (size_t)num_steps, n = (size_t)num_envs;
    const char *who = "crl_rollout_create";
    int rc = crl_dev_zalloc(&r->planes, (size_t)(num_steps + kHist) * n * kPlanePad, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->reset, tn, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->depth, tn, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->depth_carry, n, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->done, tn, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->actions, tn * 4, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->logp, tn * 4, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->values, tn * 4, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->rewards, tn * 4, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->adv, tn * 4, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->ret, tn * 4, who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->stats, kStatsDoubles<PongAdvSrc> * sizeof(double), who);
    if (rc == CRL_OK) {
        hipError_t e = hipMemset(r->depth_carry, kHist, n);  // zero history rows are physically what a fresh ring holds: depth 3
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = crl_hip_fail(e, who);
    }
    if (rc != CRL_OK) {
        crl_rollout_destroy(r);
        return rc;
    }
    *out = r;
    return CRL_OK;
}

int crl_rollout_begin(crl_rollout *r, const uint8_t *stack_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r) return crl_fail(CRL_EINVAL, "crl_rollout_begin: null storage");
    if ((uintptr_t)stack_dev & 3) return crl_fail(CRL_EINVAL, "crl_rollout_begin: the stack must be 4-byte aligned");
    if (!stack_dev && r->state == kActive)
        return crl_fail(CRL_EINVAL, "crl_rollout_begin: the rollout in progress is not finished (%d of %d steps recorded); there is nothing to carry over",
                        r->recorded, r->steps);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = r->n, row = n * kPlanePad;
    if (stack_dev) {
        hipLaunchKernelGGL(rollout_history_kernel, dim3(blocks_of(n * kHist * kPlaneWords)), dim3(256), 0, st, reinterpret_cast<uint32_t *>(r->planes),
                           reinterpret_cast<const uint32_t *>(stack_dev), n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(r->depth_carry, kHist, (size_t)n, st));
    } else if (r->state == kFinished) {
        // rows T .. T+2 become rows 0 .. 2.  Row by row and in this order a copy never reads a row an earlier one wrote (T >= 1)
        const int64_t T = r->steps;
        if (T >= kHist) HIP_TRY(hipMemcpyAsync(r->planes, r->planes + T * row, (size_t)(kHist * row), hipMemcpyDeviceToDevice, st));
        else
            for (int k = 0; k < kHist; k++) HIP_TRY(hipMemcpyAsync(r->planes + k * row, r->planes + (T + k) * row, (size_t)row, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(rollout_carry_depth_kernel, dim3(blocks_of(n)), dim3(256), 0, st, r->depth + (T - 1) * n, r->depth_carry, n);
        HIP_TRY(hipGetLastError());
    }  // (a fresh object carries its zero rows at depth 3: nothing to do)
    r->state = kActive, r->recorded = r->outcomes = 0;
    return CRL_OK;
}

int crl_rollout_record(crl_rollout *r, int64_t t, const uint8_t *frame_dev, int64_t frame_stride, const uint8_t *reset_dev, const int32_t *actions_dev,
                       int64_t action_stride, const float *values_dev, const float *logp_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !frame_dev) return crl_fail(CRL_EINVAL, "crl_rollout_record: null argument");
    if (int rc = ring_check_act("crl_rollout_record", frame_dev, frame_stride, action_stride)) return rc;
    if (((uintptr_t)actions_dev & 3) || ((uintptr_t)values_dev & 3) || ((uintptr_t)logp_dev & 3))
        return crl_fail(CRL_EINVAL, "crl_rollout_record: actions, values and log-probs must be 4-byte aligned");
    if (int rc = r->check_record("crl_rollout_record", t)) return rc;
    const int64_t n = r->n;
    RecordArgs a{frame_dev, frame_stride, reset_dev, actions_dev, action_stride, values_dev, logp_dev, t == 0 ? r->depth_carry : r->depth + (t - 1) * n,
                 reinterpret_cast<uint32_t *>(r->planes + (t + kHist) * n * kPlanePad), r->reset + t * n, r->depth + t * n, r->actions + t * n,
                 r->values + t * n, r->logp + t * n, n};
    hipLaunchKernelGGL(rollout_record_kernel, dim3(blocks_of(n * kPlaneChunks)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    r->state = kActive, r->recorded = (int)t + 1;
    return CRL_OK;
}

int crl_rollout_outcome(crl_rollout *r, int64_t t, const float *rewards_dev, int64_t reward_stride, const uint8_t *done_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !rewards_dev || !done_dev) return crl_fail(CRL_EINVAL, "crl_rollout_outcome: null argument");
    if (reward_stride < 1 || ((uintptr_t)rewards_dev & 3))
        return crl_fail(CRL_EINVAL, "crl_rollout_outcome: reward_stride must be >= 1 (float32 elements), rewards 4-byte aligned");
    if (int rc = r->check_outcome("crl_rollout_outcome", t)) return rc;
    const int64_t n = r->n;
    hipLaunchKernelGGL(rollout_outcome_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, rewards_dev, reward_stride, done_dev, r->rewards + t * n,
                       r->done + t * n, n);
    HIP_TRY(hipGetLastError());
    r->outcomes = (int)t + 1;
    return CRL_OK;
}

int crl_rollout_finish(crl_rollout *r, const float *last_values_dev, double gamma, double lam, int32_t normalize, void *stream) {
    crl_fail_no_ctx();
    if (!r) return crl_fail(CRL_EINVAL, "crl_rollout_finish: null storage");
    if ((uintptr_t)last_values_dev & 3) return crl_fail(CRL_EINVAL, "crl_rollout_finish: last_values must be 4-byte aligned");
    if (int rc = r->check_finish("crl_rollout_finish")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = r->n, tn = n * r->steps;
    const float g = (float)gamma;
    const float gl = g * (float)lam;
    hipLaunchKernelGGL(rollout_gae_kernel, dim3(blocks_of(n)), dim3(256), 0, st, r->rewards, r->values, r->done, last_values_dev, g, gl, r->adv, r->ret, n,
                       r->steps);
    HIP_TRY(hipGetLastError());
    if (normalize) HIP_TRY(rollout_stats_launch(PongAdvSrc{r->adv}, tn, r->stats, st));
    r->normalize = normalize != 0;
    r->state = kFinished;
    return CRL_OK;
}

int crl_rollout_gather(crl_rollout *r, const int64_t *idx_dev, int64_t count, void *obs_out_dev, int32_t obs_dtype, int32_t *actions_out_dev,
                       float *logp_out_dev, float *values_out_dev, float *returns_out_dev, float *adv_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !idx_dev) return crl_fail(CRL_EINVAL, "crl_rollout_gather: null argument");
    if (obs_dtype != CRL_OBS_U8 && obs_dtype != CRL_OBS_F32) return crl_fail(CRL_EINVAL, "crl_rollout_gather: obs_dtype must be CRL_OBS_U8 or CRL_OBS_F32");
    if (count < 0 || count > 0x7fffffff) return crl_fail(CRL_EINVAL, "crl_rollout_gather: the number of samples must be in [0, 2^31)");
    if (((uintptr_t)idx_dev & 7) || ((uintptr_t)obs_out_dev & (obs_dtype == CRL_OBS_F32 ? 15 : 3)) || ((uintptr_t)actions_out_dev & 3) ||
        ((uintptr_t)logp_out_dev & 3) || ((uintptr_t)values_out_dev & 3) || ((uintptr_t)returns_out_dev & 3) || ((uintptr_t)adv_out_dev & 3))
        return crl_fail(CRL_EINVAL, "crl_rollout_gather: misaligned pointer (idx 8 bytes, a float32 observation 16, everything else 4)");
    if (int rc = r->check_finished("crl_rollout_gather")) return rc;
    if (count == 0) return CRL_OK;
    GatherArgs a{reinterpret_cast<const uint32_t *>(r->planes), r->depth, idx_dev, count, (uint32_t)r->n, (uint32_t)(r->n * r->steps - 1), obs_out_dev, r->actions, r->logp, r->values, r->ret,
                 r->adv, actions_out_dev, logp_out_dev, values_out_dev, returns_out_dev, adv_out_dev, r->normalize ? r->stats : nullptr};
    const dim3 grid((unsigned)((count + 3) / 4));
    if (obs_dtype == CRL_OBS_F32) hipLaunchKernelGGL(rollout_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(rollout_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_rollout_stats(crl_rollout *r, double *out2_host) {
    crl_fail_no_ctx();
    if (!r || !out2_host) return crl_fail(CRL_EINVAL, "crl_rollout_stats: null argument");
    if (r->state != kFinished || !r->normalize)
        return crl_fail(CRL_EINVAL, "crl_rollout_stats: the statistics exist after a crl_rollout_finish that normalises");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());  // (the one call that synchronises: the finish may sit on any stream)
    HIP_TRY(hipMemcpy(out2_host, r->stats, 2 * sizeof(double), hipMemcpyDeviceToHost));
    return CRL_OK;
}

int crl_rollout_get_info(crl_rollout *r, int32_t *out4_host) {
    crl_fail_no_ctx();
    if (!r || !out4_host) return crl_fail(CRL_EINVAL, "crl_rollout_get_info: null argument");
    r->info(out4_host);
    return CRL_OK;
}

// crl_rollout_get_state (to_storage = false) and crl_rollout_set_state: the same arrays, the copies turned round.  The planes lose /
// regain their 12 bytes of padding in a pitched copy (the padding stays zero: no set ever writes it).
struct RolloutArrays {
    uint8_t *planes, *front_depth, *reset, *depth;
    int32_t *actions;
    float *logp, *values, *rewards;
    uint8_t *done;
    float *returns, *adv;
    double *stats;
};

static int rollout_copy_state(const char *who, crl_rollout *r, bool to_storage, int64_t row0, int64_t rows, int64_t steps, const RolloutArrays &x,
                              hipStream_t st) {
    const int64_t n = r->n, T = r->steps;
    if (row0 < 0 || rows < 0 || row0 + rows > T + kHist) return crl_fail(CRL_EINVAL, "%s: plane rows [%lld, %lld) outside [0, %lld]", who, (long long)row0, (long long)(row0 + rows), (long long)(T + kHist));
    if (steps < 0 || steps > T) return crl_fail(CRL_EINVAL, "%s: steps %lld outside [0, %lld]", who, (long long)steps, (long long)T);
    auto copy = [&](void *ext, void *own, size_t bytes) -> hipError_t {
        if (!ext || !bytes) return hipSuccess;
        return hipMemcpyAsync(to_storage ? own : ext, to_storage ? ext : own, bytes, hipMemcpyDeviceToDevice, st);
    };
    if (x.planes && rows) {
        uint8_t *own = r->planes + row0 * n * kPlanePad;
        const size_t plane = (size_t)kDim * kDim;
        if (to_storage) HIP_TRY(hipMemcpy2DAsync(own, kPlanePad, x.planes, plane, plane, (size_t)(rows * n), hipMemcpyDeviceToDevice, st));
        else HIP_TRY(hipMemcpy2DAsync(x.planes, plane, own, kPlanePad, plane, (size_t)(rows * n), hipMemcpyDeviceToDevice, st));
    }
    const size_t sn = (size_t)(steps * n), tn = (size_t)(T * n);
    HIP_TRY(copy(x.front_depth, r->depth_carry, (size_t)n));
    HIP_TRY(copy(x.reset, r->reset, sn));
    HIP_TRY(copy(x.depth, r->depth, sn));
    HIP_TRY(copy(x.actions, r->actions, sn * 4));
    HIP_TRY(copy(x.logp, r->logp, sn * 4));
    HIP_TRY(copy(x.values, r->values, sn * 4));
    HIP_TRY(copy(x.rewards, r->rewards, sn * 4));
    HIP_TRY(copy(x.done, r->done, sn));
    HIP_TRY(copy(x.returns, r->ret, tn * 4));
    HIP_TRY(copy(x.adv, r->adv, tn * 4));
    HIP_TRY(copy(x.stats, r->stats, 2 * sizeof(double)));
    return CRL_OK;
}

int crl_rollout_get_state(crl_rollout *r, int64_t row0, int64_t rows, uint8_t *planes_out_dev, uint8_t *front_depth_out_dev, int64_t steps,
                          uint8_t *reset_out_dev, uint8_t *depth_out_dev, int32_t *actions_out_dev, float *logp_out_dev, float *values_out_dev,
                          float *rewards_out_dev, uint8_t *done_out_dev, float *returns_out_dev, float *adv_out_dev, double *stats_out_dev,
                          void *stream) {
    crl_fail_no_ctx();
    if (!r) return crl_fail(CRL_EINVAL, "crl_rollout_get_state: null storage");
    const RolloutArrays x{planes_out_dev, front_depth_out_dev, reset_out_dev, depth_out_dev, actions_out_dev, logp_out_dev, values_out_dev,
                          rewards_out_dev, done_out_dev, returns_out_dev, adv_out_dev, stats_out_dev};
    return rollout_copy_state("crl_rollout_get_state", r, false, row0, rows, steps, x, (hipStream_t)stream);
}

int crl_rollout_set_state(crl_rollout *r, const int32_t *info4_host, int64_t row0, int64_t rows, const uint8_t *planes_dev,
                          const uint8_t *front_depth_dev, int64_t steps, const uint8_t *reset_dev, const uint8_t *depth_dev,
                          const int32_t *actions_dev, const float *logp_dev, const float *values_dev, const float *rewards_dev,
                          const uint8_t *done_dev, const float *returns_dev, const float *adv_dev, const double *stats_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !info4_host) return crl_fail(CRL_EINVAL, "crl_rollout_set_state: null argument");
    if (int rc = r->check_restore("crl_rollout_set_state", info4_host)) return rc;
    const RolloutArrays x{const_cast<uint8_t *>(planes_dev), const_cast<uint8_t *>(front_depth_dev), const_cast<uint8_t *>(reset_dev),
                          const_cast<uint8_t *>(depth_dev), const_cast<int32_t *>(actions_dev), const_cast<float *>(logp_dev),
                          const_cast<float *>(values_dev), const_cast<float *>(rewards_dev), const_cast<uint8_t *>(done_dev),
                          const_cast<float *>(returns_dev), const_cast<float *>(adv_dev), const_cast<double *>(stats_dev)};
    if (int rc = rollout_copy_state("crl_rollout_set_state", r, true, row0, rows, steps, x, (hipStream_t)stream)) return rc;
    r->restore(info4_host);
    return CRL_OK;
}

}  // extern "C"

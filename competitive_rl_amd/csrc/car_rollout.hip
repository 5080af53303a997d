// car_rollout.hip -- a CarRacing learner's rollout storage on the device (include/crl.h "car rollout storage"): T steps of what
// crl_car_policy_act wrote for the chosen cars -- the 21-float observation, the action, the value, the log-prob -- with the step's
// reward and done flag, returns and advantages by GAE, the statistics of the LIVE advantages, and the gather of a shuffled minibatch.
//
// An object beside a CarRacing context, as crl_car_policy is: it reads the context's committed per-car done flags and tile counts and
// crl_car_info's done_car itself.  One sample is one aligned 128-byte line (car_learner.h): record writes whole lines (32 lanes per
// row, one dword each, 128 contiguous bytes per row), outcome and GAE touch one line per row and step, gather and the gradient
// (car_ppo.hip) read one line per sample.
#include "car_device.h"
#include "car_learner.h"

#pragma clang fp contract(off)

namespace crl {

struct CarRecordArgs {
    const float *obs, *actions, *values, *logp;  // [N][P][21], [N][P][2], [N][P], [N][P]
    const int32_t *assign;                       // [N][P]: the policy's assignment
    const int32_t *done;                         // [P * N]: the context's per-car done flags (ci = car * N + env)
    const int32_t *ntiles;                       // [N]
    float *row;                                  // lines of step t: [R][32]
    int64_t n;
    int32_t players, cars, first, slot;  // cars = C; first = the car of column 0
};

// 32 lanes per row, one word of the line each
__global__ __launch_bounds__(256) void car_rollout_record_kernel(CarRecordArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i >> 5;
    const int w = (int)(i & 31);
    if (row >= a.n * a.cars) return;
    const int64_t e = row / a.cars;
    const int c = a.first + (int)(row - e * a.cars);
    const int64_t src = e * a.players + c;
    float v = 0.f;
    if (w < kCarLineU) v = a.obs[src * CRL_CAR_OBS_FEATURES + w];
    else if (w < kCarLineLogp) v = a.actions[src * 2 + (w - kCarLineU)];
    else if (w == kCarLineLogp) v = a.logp[src];
    else if (w == kCarLineValue) v = a.values[src];
    else if (w == kCarLineFlags) {
        const bool live = a.assign[src] == a.slot && a.done[(int64_t)c * a.n + e] == 0 && a.ntiles[e] > 0;
        v = __uint_as_float(live ? kCarFlagLive : 0u);
    }
    a.row[row * kCarLineWords + w] = v;
}

// a lane per row: the reward and the row's done flag = done[e] != 0 || done_car[e][c] != 0
__global__ __launch_bounds__(256) void car_rollout_outcome_kernel(const float *__restrict__ rewards, const uint8_t *__restrict__ done,
                                                                 const uint8_t *__restrict__ done_car, float *__restrict__ rowp, int64_t n, int players,
                                                                 int cars, int first) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n * cars) return;
    const int64_t e = row / cars;
    const int c = first + (int)(row - e * cars);
    float *line = rowp + row * kCarLineWords;
    line[kCarLineReward] = rewards[e * players + c];
    const uint32_t fl = __float_as_uint(line[kCarLineFlags]) & kCarFlagLive;
    const bool d = done[e] != 0 || done_car[e * players + c] != 0;
    line[kCarLineFlags] = __uint_as_float(fl | (d ? kCarFlagDone : 0u));
}

// include/crl.h "GAE rule" (rollout_core.h): a lane per row walks t = T-1 .. 0 over the rows' lines
__global__ __launch_bounds__(256) void car_rollout_gae_kernel(float *__restrict__ lines, const float *__restrict__ last_values, float g, float gl, int64_t n,
                                                             int players, int cars, int first, int steps) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rows = n * cars;
    if (row >= rows) return;
    const int64_t e = row / cars;
    const int c = first + (int)(row - e * cars);
    float acc = 0.0f;
    float vnext = last_values ? last_values[e * players + c] : 0.0f;
    for (int t = steps - 1; t >= 0; t--) {
        float *line = lines + ((int64_t)t * rows + row) * kCarLineWords;
        const bool done = (__float_as_uint(line[kCarLineFlags]) & kCarFlagDone) != 0;
        gae_step(line[kCarLineReward], line[kCarLineValue], done, g, gl, acc, vnext, line[kCarLineAdv], line[kCarLineReturn]);
    }
}

struct CarAdvSrc {  // the statistics' source (rollout_core.h): the advantages of the LIVE samples, stats[2] = their count L
    static constexpr bool kCounted = true;
    const float *__restrict__ lines;
    __device__ bool live(int64_t i) const { return (__float_as_uint(lines[i * kCarLineWords + kCarLineFlags]) & kCarFlagLive) != 0; }
    __device__ float adv(int64_t i) const { return lines[i * kCarLineWords + kCarLineAdv]; }
};

struct CarGatherArgs {
    const float *lines;
    const int64_t *idx;
    int64_t count;
    uint32_t last;
    float *obs, *actions, *logp, *values, *ret, *adv;  // each optional
    uint8_t *live;
    const double *stats;  // read when the advantages are normalised, else null
};

// 32 lanes per sample: one coalesced read of the sample's line, each lane stores its word where it belongs
__global__ __launch_bounds__(256) void car_rollout_gather_kernel(CarGatherArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b = i >> 5;
    const int w = (int)(i & 31);
    if (b >= a.count) return;
    // (the indices' validity is the caller's; the clamp only keeps a bad one's READS inside the array)
    const uint32_t raw = (uint32_t)a.idx[b];
    const uint32_t flat = raw < a.last ? raw : a.last;
    const float v = a.lines[(int64_t)flat * kCarLineWords + w];
    if (w < kCarLineU) {
        if (a.obs) a.obs[b * CRL_CAR_OBS_FEATURES + w] = v;
    } else if (w < kCarLineLogp) {
        if (a.actions) a.actions[b * 2 + (w - kCarLineU)] = v;
    } else if (w == kCarLineLogp) {
        if (a.logp) a.logp[b] = v;
    } else if (w == kCarLineValue) {
        if (a.values) a.values[b] = v;
    } else if (w == kCarLineReturn) {
        if (a.ret) a.ret[b] = v;
    } else if (w == kCarLineAdv) {
        if (a.adv) a.adv[b] = adv_out(v, a.stats);
    } else if (w == kCarLineFlags) {
        if (a.live) a.live[b] = (uint8_t)(__float_as_uint(v) & kCarFlagLive);
    }
}

}  // namespace crl

using namespace crl;

struct crl_car_rollout : RolloutSteps {
    crl_car_ctx *car = nullptr;
    int64_t n = 0;
    int players = 0, cars = 0, first = 0, mask = 0;
    float *lines = nullptr;      // [T * R][32]
    int32_t *assign = nullptr;   // [N][players]: the policy's assignment at the last record
    double *stats = nullptr;     // mean, std, L, then kRedGroups partial sums and kRedGroups partial counts (kStatsDoubles)
};

namespace crl {
CarRolloutView car_rollout_view(const ::crl_car_rollout *r) {
    return CarRolloutView{r->lines, r->normalize ? r->stats : nullptr, (uint32_t)(r->n * r->cars * r->steps - 1), r->state == kFinished};
}
}  // namespace crl

extern "C" {

void crl_car_rollout_destroy(crl_car_rollout *r) {
    if (!r) return;
    for (void *p : {(void *)r->lines, (void *)r->assign, (void *)r->stats})
        if (p) (void)hipFree(p);
    delete r;
}

int crl_car_rollout_create(crl_ctx *ctx, int64_t num_steps, int32_t cars_mask, crl_car_rollout **out) {
    crl_fail_no_ctx();
    if (!ctx || !out) return crl_fail(CRL_EINVAL, "crl_car_rollout_create: null argument");
    crl_car_ctx *car = crl_ctx_car(ctx);
    if (!car) return crl_fail(CRL_EINVAL, "crl_car_rollout_create: not a CarRacing context");
    const CarSoA *s = crl_car_soa(car);
    if (cars_mask < 1 || cars_mask > 3 || (cars_mask & 2 && s->players < 2))
        return crl_fail(CRL_EINVAL, "crl_car_rollout_create: cars_mask %d names no car, or a car the context lacks (%d players)", cars_mask, s->players);
    const int cars = cars_mask == 3 ? 2 : 1;
    if (num_steps <= 0 || num_steps > 0x7fffffff || (int64_t)s->n * cars > 0x7fffffff / num_steps)
        return crl_fail(CRL_EINVAL, "crl_car_rollout_create: num_steps >= 1 and num_steps * rows < 2^31 are needed");
    *out = nullptr;
    crl_car_rollout *r = new crl_car_rollout();
    r->car = car, r->n = s->n, r->players = s->players, r->cars = cars, r->first = cars_mask == 2 ? 1 : 0, r->mask = cars_mask, r->steps = (int)num_steps;
    const char *who = "crl_car_rollout_create";
    int rc = crl_dev_zalloc(&r->lines, (size_t)num_steps * r->n * cars * kCarLineWords * sizeof(float), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->assign, (size_t)r->n * r->players * sizeof(int32_t), who);
    if (rc == CRL_OK) rc = crl_dev_zalloc(&r->stats, kStatsDoubles<CarAdvSrc> * sizeof(double), who);
    if (rc == CRL_OK) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = crl_hip_fail(e, who);
    }
    if (rc != CRL_OK) {
        crl_car_rollout_destroy(r);
        return rc;
    }
    *out = r;
    return CRL_OK;
}

int crl_car_rollout_begin(crl_car_rollout *r) {
    crl_fail_no_ctx();
    if (!r) return crl_fail(CRL_EINVAL, "crl_car_rollout_begin: null storage");
    r->state = kActive, r->recorded = r->outcomes = 0;
    return CRL_OK;
}

int crl_car_rollout_record(crl_car_rollout *r, int64_t t, crl_car_policy *policy, int32_t slot, const float *obs_dev, const float *actions_dev,
                           const float *values_dev, const float *log_probs_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !policy || !obs_dev || !actions_dev || !values_dev || !log_probs_dev) return crl_fail(CRL_EINVAL, "crl_car_rollout_record: null argument");
    if (((uintptr_t)obs_dev | (uintptr_t)actions_dev | (uintptr_t)values_dev | (uintptr_t)log_probs_dev) & 3)
        return crl_fail(CRL_EINVAL, "crl_car_rollout_record: the tensors must be 4-byte aligned");
    if (int rc = r->check_record("crl_car_rollout_record", t)) return rc;
    int32_t flag = 0;
    if (int rc = crl_car_policy_get_weights(policy, slot, nullptr, &flag, nullptr)) return rc;  // (refuses a bad or an empty slot)
    if (flag != 0) return crl_fail(CRL_EINVAL, "crl_car_rollout_record: slot %d is deterministic: its log-probs are 0, which is not training material", slot);
    if (int rc = crl_car_policy_get_assignment(policy, r->assign, stream)) return rc;
    const CarSoA *s = crl_car_soa(r->car);
    const int64_t rows = r->n * r->cars;
    CarRecordArgs a{obs_dev, actions_dev, values_dev, log_probs_dev, r->assign, s->done, s->ntiles, r->lines + t * rows * kCarLineWords,
                    r->n,    r->players,  r->cars,    r->first,      slot};
    hipLaunchKernelGGL(car_rollout_record_kernel, dim3(blocks_of(rows * kCarLineWords)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    r->state = kActive, r->recorded = (int)t + 1;
    return CRL_OK;
}

int crl_car_rollout_outcome(crl_car_rollout *r, int64_t t, const float *rewards_dev, const uint8_t *done_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !rewards_dev || !done_dev) return crl_fail(CRL_EINVAL, "crl_car_rollout_outcome: null argument");
    if ((uintptr_t)rewards_dev & 3) return crl_fail(CRL_EINVAL, "crl_car_rollout_outcome: rewards must be 4-byte aligned");
    if (int rc = r->check_outcome("crl_car_rollout_outcome", t)) return rc;
    const int64_t rows = r->n * r->cars;
    hipLaunchKernelGGL(car_rollout_outcome_kernel, dim3(blocks_of(rows)), dim3(256), 0, (hipStream_t)stream, rewards_dev, done_dev, crl_car_done_flags(r->car),
                       r->lines + t * rows * kCarLineWords, r->n, r->players, r->cars, r->first);
    HIP_TRY(hipGetLastError());
    r->outcomes = (int)t + 1;
    return CRL_OK;
}

int crl_car_rollout_finish(crl_car_rollout *r, const float *last_values_dev, double gamma, double lam, int32_t normalize, void *stream) {
    crl_fail_no_ctx();
    if (!r) return crl_fail(CRL_EINVAL, "crl_car_rollout_finish: null storage");
    if ((uintptr_t)last_values_dev & 3) return crl_fail(CRL_EINVAL, "crl_car_rollout_finish: last_values must be 4-byte aligned");
    if (int rc = r->check_finish("crl_car_rollout_finish")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = r->n * r->cars, total = rows * r->steps;
    const float g = (float)gamma;
    const float gl = g * (float)lam;
    hipLaunchKernelGGL(car_rollout_gae_kernel, dim3(blocks_of(rows)), dim3(256), 0, st, r->lines, last_values_dev, g, gl, r->n, r->players, r->cars, r->first,
                       r->steps);
    HIP_TRY(hipGetLastError());
    if (normalize) HIP_TRY(rollout_stats_launch(CarAdvSrc{r->lines}, total, r->stats, st));
    r->normalize = normalize != 0;
    r->state = kFinished;
    return CRL_OK;
}

int crl_car_rollout_gather(crl_car_rollout *r, const int64_t *idx_dev, int64_t count, float *obs_out_dev, float *actions_out_dev, float *logp_out_dev,
                           float *values_out_dev, float *returns_out_dev, float *adv_out_dev, uint8_t *live_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !idx_dev) return crl_fail(CRL_EINVAL, "crl_car_rollout_gather: null argument");
    if (count < 0 || count > 0x7fffffff / kCarLineWords) return crl_fail(CRL_EINVAL, "crl_car_rollout_gather: the number of samples must be in [0, 2^26)");
    if (((uintptr_t)idx_dev & 7) || (((uintptr_t)obs_out_dev | (uintptr_t)actions_out_dev | (uintptr_t)logp_out_dev | (uintptr_t)values_out_dev |
                                      (uintptr_t)returns_out_dev | (uintptr_t)adv_out_dev) & 3))
        return crl_fail(CRL_EINVAL, "crl_car_rollout_gather: misaligned pointer (idx 8 bytes, every float32 output 4)");
    if (int rc = r->check_finished("crl_car_rollout_gather")) return rc;
    if (count == 0) return CRL_OK;
    CarGatherArgs a{r->lines,       idx_dev,         count,       (uint32_t)(r->n * r->cars * r->steps - 1), obs_out_dev, actions_out_dev, logp_out_dev,
                    values_out_dev, returns_out_dev, adv_out_dev, live_out_dev,                              r->normalize ? r->stats : nullptr};
    hipLaunchKernelGGL(car_rollout_gather_kernel, dim3(blocks_of(count * kCarLineWords)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_car_rollout_stats(crl_car_rollout *r, double *out3_host) {
    crl_fail_no_ctx();
    if (!r || !out3_host) return crl_fail(CRL_EINVAL, "crl_car_rollout_stats: null argument");
    if (r->state != kFinished || !r->normalize)
        return crl_fail(CRL_EINVAL, "crl_car_rollout_stats: the statistics exist after a crl_car_rollout_finish that normalises");
    HIP_TRY(hipDeviceSynchronize());  // (the one call that synchronises: the finish may sit on any stream)
    HIP_TRY(hipMemcpy(out3_host, r->stats, 3 * sizeof(double), hipMemcpyDeviceToHost));
    return CRL_OK;
}

int crl_car_rollout_get_info(crl_car_rollout *r, int32_t *out8_host) {
    crl_fail_no_ctx();
    if (!r || !out8_host) return crl_fail(CRL_EINVAL, "crl_car_rollout_get_info: null argument");
    r->info(out8_host);
    out8_host[4] = r->steps, out8_host[5] = r->cars, out8_host[6] = r->mask, out8_host[7] = kCarLineWords;
    return CRL_OK;
}

int crl_car_rollout_get_state(crl_car_rollout *r, int64_t steps, float *lines_out_dev, double *stats_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r) return crl_fail(CRL_EINVAL, "crl_car_rollout_get_state: null storage");
    if (steps < 0 || steps > r->steps) return crl_fail(CRL_EINVAL, "crl_car_rollout_get_state: steps %lld outside [0, %d]", (long long)steps, r->steps);
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)steps * r->n * r->cars * kCarLineWords * sizeof(float);
    if (lines_out_dev && bytes) HIP_TRY(hipMemcpyAsync(lines_out_dev, r->lines, bytes, hipMemcpyDeviceToDevice, st));
    if (stats_out_dev) HIP_TRY(hipMemcpyAsync(stats_out_dev, r->stats, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return CRL_OK;
}

int crl_car_rollout_set_state(crl_car_rollout *r, const int32_t *info4_host, int64_t steps, const float *lines_dev, const double *stats_dev, void *stream) {
    crl_fail_no_ctx();
    if (!r || !info4_host) return crl_fail(CRL_EINVAL, "crl_car_rollout_set_state: null argument");
    if (int rc = r->check_restore("crl_car_rollout_set_state", info4_host)) return rc;
    if (steps < 0 || steps > r->steps) return crl_fail(CRL_EINVAL, "crl_car_rollout_set_state: steps %lld outside [0, %d]", (long long)steps, r->steps);
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)steps * r->n * r->cars * kCarLineWords * sizeof(float);
    if (lines_dev && bytes) HIP_TRY(hipMemcpyAsync(r->lines, lines_dev, bytes, hipMemcpyDeviceToDevice, st));
    if (stats_dev) HIP_TRY(hipMemcpyAsync(r->stats, stats_dev, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    r->restore(info4_host);
    return CRL_OK;
}

}  // extern "C"

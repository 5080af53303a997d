// pong_ledger.hip -- the league's results ledger: how the learner fares against every agent of a crl_league's pool, and the draw of
// the next opponent weighted by it (include/crl.h "league ledger", "ledger draws", "PFSP weights").  An object beside crl_league:
// nothing here reaches into a league, the caller passes the assignment in and takes the new ids out.
//
// Stands in for the bookkeeping a league trainer around the reference's TournamentEnvWrapper does on the host (episode returns per
// current_agent, competitive_pong_env.py:27-41 has no such record itself): here it is one launch per step with one lane per env.
// Episode ends are rare (one step in several hundred per env), so a wavefront without one leaves after its loads and stores; one
// with some reduces them per agent (ballot + popcount, a shuffle tree for the two sums) and its leader adds with six 64-bit
// atomics per agent.  Integer sums: the totals do not depend on arrival order.
#include "crl_internal.h"
#include "pong_device.h"

namespace crl {

static constexpr int kGThreads = 256;
static constexpr int kGAgents = CRL_LEAGUE_MAX_AGENTS;
static constexpr int kGCounters = CRL_LEDGER_COUNTERS * kGAgents;  // int64 words; `ignored` is word kGCounters

struct LedgerTable {
    uint32_t w[kGAgents];
};

__device__ inline long long wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// include/crl.h "ledger draws": the smallest a whose cumulative weight exceeds (x0 * T) >> 32; -1 when the table sums to 0 (or past 2^32)
__device__ inline int ledger_draw(const uint32_t *__restrict__ w, uint64_t seed, uint64_t gid, uint32_t n) {
    uint64_t total = 0;
#pragma unroll
    for (int a = 0; a < kGAgents; a++) total += w[a];
    if (total - 1 >= 0xFFFFFFFFull) return -1;
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), n, CRL_LEDGER_DOMAIN_OPPONENT};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t r = ((uint64_t)c[0] * total) >> 32;
    uint64_t cum = 0;
    int drawn = -1;
#pragma unroll
    for (int a = 0; a < kGAgents; a++) {
        cum += w[a];
        if (drawn < 0 && cum > r) drawn = a;
    }
    return drawn;
}

__global__ __launch_bounds__(kGThreads) void ledger_step_kernel(int agents, const int32_t *assign, const float *__restrict__ reward,
                                                               int64_t reward_stride, const uint8_t *__restrict__ done, int redraw,
                                                               int32_t *__restrict__ ret, int32_t *__restrict__ len, uint32_t *__restrict__ draw_ctr,
                                                               unsigned long long *__restrict__ counters, const uint32_t *__restrict__ w, uint64_t seed,
                                                               int64_t env_id_base, int64_t n, int32_t *ids_out) {
    const int64_t i = (int64_t)blockIdx.x * kGThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int credit = -1;  // the agent this lane's finished episode goes to; -2: an id outside the pool; -1: no episode ended here
    int r = 0, steps = 0;
    if (i < n) {
        const int a = assign[i];
        r = ret[i] + (int)reward[i * reward_stride];
        steps = len[i] + 1;
        const bool d = done[i] != 0;
        int id = a;
        if (d) {
            credit = (a >= 0 && a < agents) ? a : -2;
            if (redraw) {
                const uint32_t ctr = draw_ctr[i];
                const int drawn = ledger_draw(w, seed, (uint64_t)(env_id_base + i), ctr);
                if (drawn >= 0) id = drawn, draw_ctr[i] = ctr + 1;
            }
        }
        ret[i] = d ? 0 : r, len[i] = d ? 0 : steps;
        ids_out[i] = id;
    }
    if (!__ballot(credit != -1)) return;  // (uniform) the usual case: no episode of this wavefront ended
    for (int k = 0; k < agents; k++) {
        const bool mine = credit == k;
        const unsigned long long m = __ballot(mine);
        if (!m) continue;  // (uniform)
        const unsigned long long won = __ballot(mine && r > 0), lost = __ballot(mine && r < 0);
        const long long ret_sum = wave_sum(mine ? (long long)r : 0ll), len_sum = wave_sum(mine ? (long long)steps : 0ll);
        if (lane == __ffsll(m) - 1) {
            const unsigned long long e = (unsigned long long)__popcll(m), nw = (unsigned long long)__popcll(won), nl = (unsigned long long)__popcll(lost);
            atomicAdd(&counters[CRL_LEDGER_EPISODES * kGAgents + k], e);
            if (nw) atomicAdd(&counters[CRL_LEDGER_WINS * kGAgents + k], nw);
            if (nl) atomicAdd(&counters[CRL_LEDGER_LOSSES * kGAgents + k], nl);
            if (e - nw - nl) atomicAdd(&counters[CRL_LEDGER_DRAWS * kGAgents + k], e - nw - nl);
            atomicAdd(&counters[CRL_LEDGER_RETURN_SUM * kGAgents + k], (unsigned long long)ret_sum);
            atomicAdd(&counters[CRL_LEDGER_LENGTH_SUM * kGAgents + k], (unsigned long long)len_sum);
        }
    }
    const unsigned long long stray = __ballot(credit == -2);
    if (stray && lane == __ffsll(stray) - 1) atomicAdd(&counters[kGCounters], (unsigned long long)__popcll(stray));
}

// include/crl.h "PFSP weights": lane a of one wavefront, float64 with one rounding per operation (-ffp-contract=off)
__global__ __launch_bounds__(64) void ledger_pfsp_kernel(const long long *__restrict__ counters, int agents, int mode, int exponent, uint32_t floor_w,
                                                        uint32_t *__restrict__ w) {
    const int a = threadIdx.x;
    if (a >= kGAgents) return;
    uint32_t out = 0;
    if (a < agents) {
        const double episodes = (double)counters[CRL_LEDGER_EPISODES * kGAgents + a], wins = (double)counters[CRL_LEDGER_WINS * kGAgents + a];
        const double draws = (double)counters[CRL_LEDGER_DRAWS * kGAgents + a];
        const double p = ((wins + 0.5 * draws) + 1.0) / (episodes + 2.0);
        const double q = 1.0 - p;
        double f = q;
        if (mode == CRL_LEDGER_PFSP_VARIANCE) f = p * q;
        else
            for (int j = 1; j < exponent; j++) f = f * q;
        out = floor_w + (uint32_t)floor(f * 65535.0);
    }
    w[a] = out;
}

__global__ void ledger_set_weights_kernel(LedgerTable t, uint32_t *__restrict__ w) {
    if (threadIdx.x < kGAgents) w[threadIdx.x] = t.w[threadIdx.x];
}

// rows that enter the pool get weight 1, rows that leave it weight 0
__global__ void ledger_resize_kernel(int before, int after, uint32_t *__restrict__ w) {
    const int a = threadIdx.x;
    if (a >= kGAgents) return;
    if (a >= after) w[a] = 0;
    else if (a >= before) w[a] = 1;
}

}  // namespace crl

using namespace crl;

struct crl_ledger {
    int device = 0;
    int64_t n = 0, env_id_base = 0;
    uint64_t seed = 0;
    int agents = 0;
    int32_t *ret = nullptr, *len = nullptr;
    uint32_t *draw_ctr = nullptr;
    unsigned long long *counters = nullptr;  // [CRL_LEDGER_COUNTERS][kGAgents], then `ignored`
    uint32_t *w = nullptr;                   // [kGAgents]
};

static int ledger_copy(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (dst && src) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return CRL_OK;
}

extern "C" {

int crl_ledger_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int32_t agents, crl_ledger **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || num_envs > 0x7fffffff || env_id_base < 0 || agents < 1 || agents > kGAgents)
        return crl_fail(CRL_EINVAL, "crl_ledger_create: bad arguments (num_envs in [1, 2^31), env_id_base >= 0, agents in [1, %d])", kGAgents);
    HIP_TRY(hipSetDevice(device));
    crl_ledger *l = new crl_ledger();
    l->device = device, l->n = num_envs, l->env_id_base = env_id_base, l->seed = seed, l->agents = agents;
    const size_t per_env = (size_t)num_envs * sizeof(int32_t), books = (kGCounters + 1) * sizeof(unsigned long long);
    const char *what = "crl_ledger_create";
    int rc = crl_dev_zalloc(&l->ret, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&l->len, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&l->draw_ctr, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&l->counters, books, what);
    if (!rc) rc = crl_dev_zalloc(&l->w, kGAgents * sizeof(uint32_t), what);
    if (!rc) {
        hipLaunchKernelGGL(ledger_resize_kernel, dim3(1), dim3(64), 0, nullptr, 0, agents, l->w);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = crl_hip_fail(e, what);
    }
    if (rc) {
        crl_ledger_destroy(l);
        return rc;
    }
    *out = l;
    return CRL_OK;
}

void crl_ledger_destroy(crl_ledger *l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    if (l->ret) (void)hipFree(l->ret);
    if (l->len) (void)hipFree(l->len);
    if (l->draw_ctr) (void)hipFree(l->draw_ctr);
    if (l->counters) (void)hipFree(l->counters);
    if (l->w) (void)hipFree(l->w);
    delete l;
}

int crl_ledger_seed(crl_ledger *l, uint64_t seed, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_seed: null ledger");
    HIP_TRY(hipMemsetAsync(l->draw_ctr, 0, (size_t)l->n * sizeof(uint32_t), (hipStream_t)stream));
    l->seed = seed;
    return CRL_OK;
}

int crl_ledger_reset(crl_ledger *l, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_reset: null ledger");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(l->counters, 0, (kGCounters + 1) * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(l->ret, 0, (size_t)l->n * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(l->len, 0, (size_t)l->n * sizeof(int32_t), st));
    return CRL_OK;
}

int crl_ledger_set_agents(crl_ledger *l, int32_t agents, void *stream) {
    crl_fail_no_ctx();
    if (!l || agents < 1 || agents > kGAgents) return crl_fail(CRL_EINVAL, "crl_ledger_set_agents: agents must be in [1, %d]", kGAgents);
    hipLaunchKernelGGL(ledger_resize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, l->agents, agents, l->w);
    HIP_TRY(hipGetLastError());
    l->agents = agents;
    return CRL_OK;
}

int crl_ledger_set_weights(crl_ledger *l, const uint32_t *w_host, int32_t count, void *stream) {
    crl_fail_no_ctx();
    if (!l || !w_host) return crl_fail(CRL_EINVAL, "crl_ledger_set_weights: null argument");
    if (count != l->agents) return crl_fail(CRL_EINVAL, "crl_ledger_set_weights: %d weights for a pool of %d agents", count, l->agents);
    LedgerTable t{};
    uint64_t total = 0;
    for (int a = 0; a < count; a++) t.w[a] = w_host[a], total += w_host[a];
    if (total == 0 || total >= (1ull << 32))
        return crl_fail(CRL_EINVAL, "crl_ledger_set_weights: the weights must sum to a value in [1, 2^32), not %llu", (unsigned long long)total);
    hipLaunchKernelGGL(ledger_set_weights_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t, l->w);  // (the table travels as kernel arguments)
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_ledger_get_weights(crl_ledger *l, uint32_t *w_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !w_out_dev) return crl_fail(CRL_EINVAL, "crl_ledger_get_weights: null argument");
    return ledger_copy(w_out_dev, l->w, kGAgents * sizeof(uint32_t), (hipStream_t)stream);
}

int crl_ledger_pfsp_weights(crl_ledger *l, const int64_t *counters_dev, int32_t mode, int32_t exponent, uint32_t floor, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_pfsp_weights: null ledger");
    if (mode != CRL_LEDGER_PFSP_HARD && mode != CRL_LEDGER_PFSP_VARIANCE)
        return crl_fail(CRL_EINVAL, "crl_ledger_pfsp_weights: mode must be CRL_LEDGER_PFSP_HARD or CRL_LEDGER_PFSP_VARIANCE");
    if (mode == CRL_LEDGER_PFSP_HARD && (exponent < 1 || exponent > 64)) return crl_fail(CRL_EINVAL, "crl_ledger_pfsp_weights: exponent must be in [1, 64]");
    if ((uint64_t)l->agents * ((uint64_t)floor + 65535u) >= (1ull << 32))
        return crl_fail(CRL_EINVAL, "crl_ledger_pfsp_weights: floor %u lets the weights of %d agents sum past 2^32", floor, l->agents);
    const long long *src = counters_dev ? reinterpret_cast<const long long *>(counters_dev) : reinterpret_cast<const long long *>(l->counters);
    hipLaunchKernelGGL(ledger_pfsp_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src, l->agents, mode, exponent, floor, l->w);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_ledger_get_counters(crl_ledger *l, int64_t *counters_out_dev, int64_t *ignored_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counters_out_dev) return crl_fail(CRL_EINVAL, "crl_ledger_get_counters: null argument");
    int rc = ledger_copy(counters_out_dev, l->counters, kGCounters * sizeof(int64_t), (hipStream_t)stream);
    return rc != CRL_OK ? rc : ledger_copy(ignored_out_dev, l->counters + kGCounters, sizeof(int64_t), (hipStream_t)stream);
}

int crl_ledger_set_counters(crl_ledger *l, const int64_t *counters_dev, const int64_t *ignored_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counters_dev) return crl_fail(CRL_EINVAL, "crl_ledger_set_counters: null argument");
    int rc = ledger_copy(l->counters, counters_dev, kGCounters * sizeof(int64_t), (hipStream_t)stream);
    return rc != CRL_OK ? rc : ledger_copy(l->counters + kGCounters, ignored_dev, sizeof(int64_t), (hipStream_t)stream);
}

int crl_ledger_get_env_state(crl_ledger *l, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_get_env_state: null ledger");
    const size_t bytes = (size_t)l->n * sizeof(int32_t);
    int rc = ledger_copy(ret_out_dev, l->ret, bytes, (hipStream_t)stream);
    if (rc == CRL_OK) rc = ledger_copy(len_out_dev, l->len, bytes, (hipStream_t)stream);
    return rc != CRL_OK ? rc : ledger_copy(draw_ctr_out_dev, l->draw_ctr, bytes, (hipStream_t)stream);
}

int crl_ledger_set_env_state(crl_ledger *l, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_set_env_state: null ledger");
    const size_t bytes = (size_t)l->n * sizeof(int32_t);
    int rc = ledger_copy(l->ret, ret_dev, bytes, (hipStream_t)stream);
    if (rc == CRL_OK) rc = ledger_copy(l->len, len_dev, bytes, (hipStream_t)stream);
    return rc != CRL_OK ? rc : ledger_copy(l->draw_ctr, draw_ctr_dev, bytes, (hipStream_t)stream);
}

int crl_ledger_step(crl_ledger *l, const int32_t *assign_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev,
                    int32_t redraw, int32_t *ids_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !assign_dev || !reward_dev || !done_dev || !ids_out_dev) return crl_fail(CRL_EINVAL, "crl_ledger_step: null argument");
    if (reward_stride < 1) return crl_fail(CRL_EINVAL, "crl_ledger_step: reward_stride must be >= 1 (float32 elements)");
    hipLaunchKernelGGL(ledger_step_kernel, dim3((unsigned)((l->n + kGThreads - 1) / kGThreads)), dim3(kGThreads), 0, (hipStream_t)stream, l->agents,
                       assign_dev, reward_dev, reward_stride, done_dev, redraw, l->ret, l->len, l->draw_ctr, l->counters, l->w, l->seed, l->env_id_base,
                       l->n, ids_out_dev);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

}  // extern "C"

// pong_ledger.hip -- the league's results ledger: how the learner fares against every agent of a crl_league's pool, and the draw of
// the next opponent weighted by it (include/crl.h "league ledger", "ledger draws", "PFSP weights").  An object beside crl_league:
// nothing here reaches into a league, the caller passes the assignment in and takes the new ids out.
//
// Stands in for the bookkeeping a league trainer around the reference's TournamentEnvWrapper does on the host (episode returns per
// current_agent, competitive_pong_env.py:27-41 has no such record itself): here it is one launch per step with one lane per env,
// books_step_kernel of pong_books.h keyed by the opponent's id.  This file holds what knows that key and the entry points; lifetime,
// seed, reset and the copies are the shared Books'.  The writers of a table of one weight per agent (set weights, PFSP) are defined here
// for the CarRacing league's table as well (pong_books.h declares them).
#include "pong_books.h"

namespace crl {

static constexpr int kGAgents = kBAgents;
static constexpr int kGCounters = kBPlanes * kGAgents;  // int64 words; `ignored` is word kGCounters

struct Table16 {
    uint32_t w[kGAgents];
};

struct LedgerTraits {
    static constexpr int kIds = 1, kKeys = kGAgents;
    static __device__ int key(const int32_t *ids, int agents) { return (ids[0] >= 0 && ids[0] < agents) ? ids[0] : -2; }
    static __device__ int draw(const uint32_t *__restrict__ w, uint64_t seed, uint64_t gid, uint32_t n) {
        return books_draw16(w, seed, gid, n, CRL_LEDGER_DOMAIN_OPPONENT);
    }
    static __device__ void put(int key, int32_t *ids) { ids[0] = key; }
};

// include/crl.h "PFSP weights" over counter planes of kGAgents words (the ledger's, the car league's: episodes, wins and draws are
// planes 0, 1, 3 of both): lane a of one wavefront, float64 with one rounding per operation (-ffp-contract=off)
__global__ __launch_bounds__(64) void books_pfsp16_kernel(const long long *__restrict__ counters, int agents, int mode, int exponent, uint32_t floor_w,
                                                         uint32_t *__restrict__ w) {
    const int a = threadIdx.x;
    if (a >= kGAgents) return;
    uint32_t out = 0;
    if (a < agents) {
        const double episodes = (double)counters[kBEpisodes * kGAgents + a], wins = (double)counters[kBWins * kGAgents + a];
        const double draws = (double)counters[kBDraws * kGAgents + a];
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

__global__ void books_set_weights16_kernel(Table16 t, uint32_t *__restrict__ w) {
    if (threadIdx.x < kGAgents) w[threadIdx.x] = t.w[threadIdx.x];
}

// rows that enter the pool get weight 1, rows that leave it weight 0
__global__ void ledger_resize_kernel(int before, int after, uint32_t *__restrict__ w) {
    const int a = threadIdx.x;
    if (a >= kGAgents) return;
    if (a >= after) w[a] = 0;
    else if (a >= before) w[a] = 1;
}

int books_set_weights16(const char *who, uint32_t *w, int agents, const uint32_t *w_host, int32_t count, hipStream_t st) {
    if (count != agents || count < 1) return crl_fail(CRL_EINVAL, "%s: %d weights for a pool of %d agents", who, count, agents);
    Table16 t{};
    uint64_t total = 0;
    for (int a = 0; a < count; a++) t.w[a] = w_host[a], total += w_host[a];
    if (total == 0 || total >= (1ull << 32))
        return crl_fail(CRL_EINVAL, "%s: the weights must sum to a value in [1, 2^32), not %llu", who, (unsigned long long)total);
    hipLaunchKernelGGL(books_set_weights16_kernel, dim3(1), dim3(64), 0, st, t, w);  // (the table travels as kernel arguments)
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int books_pfsp16(const char *who, uint32_t *w, int agents, const unsigned long long *own, const int64_t *counters_dev, int32_t mode, int32_t exponent,
                 uint32_t floor, hipStream_t st) {
    if (mode != CRL_LEDGER_PFSP_HARD && mode != CRL_LEDGER_PFSP_VARIANCE)
        return crl_fail(CRL_EINVAL, "%s: mode must be CRL_LEDGER_PFSP_HARD or CRL_LEDGER_PFSP_VARIANCE", who);
    if (mode == CRL_LEDGER_PFSP_HARD && (exponent < 1 || exponent > 64)) return crl_fail(CRL_EINVAL, "%s: exponent must be in [1, 64]", who);
    if ((uint64_t)agents * ((uint64_t)floor + 65535u) >= (1ull << 32))
        return crl_fail(CRL_EINVAL, "%s: floor %u lets the weights of %d agents sum past 2^32", who, floor, agents);
    const long long *src = counters_dev ? reinterpret_cast<const long long *>(counters_dev) : reinterpret_cast<const long long *>(own);
    hipLaunchKernelGGL(books_pfsp16_kernel, dim3(1), dim3(64), 0, st, src, agents, mode, exponent, floor, w);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

}  // namespace crl

using namespace crl;

struct crl_ledger : Books {};  // counters [CRL_LEDGER_COUNTERS][kGAgents], then `ignored`; w [kGAgents]

extern "C" {

int crl_ledger_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int32_t agents, crl_ledger **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || num_envs > 0x7fffffff || env_id_base < 0 || agents < 1 || agents > kGAgents)
        return crl_fail(CRL_EINVAL, "crl_ledger_create: bad arguments (num_envs in [1, 2^31), env_id_base >= 0, agents in [1, %d])", kGAgents);
    return books_create("crl_ledger_create", device, num_envs, env_id_base, seed, agents, kGCounters, kGAgents,
                        [](uint32_t *w, int pool) { hipLaunchKernelGGL(ledger_resize_kernel, dim3(1), dim3(64), 0, nullptr, 0, pool, w); }, out);
}

void crl_ledger_destroy(crl_ledger *l) { books_destroy(l); }

int crl_ledger_seed(crl_ledger *l, uint64_t seed, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_seed: null ledger");
    return books_seed(l, seed, (hipStream_t)stream);
}

int crl_ledger_reset(crl_ledger *l, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_reset: null ledger");
    return books_reset(l, (hipStream_t)stream);
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
    return books_set_weights16("crl_ledger_set_weights", l->w, l->agents, w_host, count, (hipStream_t)stream);
}

int crl_ledger_get_weights(crl_ledger *l, uint32_t *w_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !w_out_dev) return crl_fail(CRL_EINVAL, "crl_ledger_get_weights: null argument");
    return books_get_weights(l, w_out_dev, kGAgents, (hipStream_t)stream);
}

int crl_ledger_pfsp_weights(crl_ledger *l, const int64_t *counters_dev, int32_t mode, int32_t exponent, uint32_t floor, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_pfsp_weights: null ledger");
    return books_pfsp16("crl_ledger_pfsp_weights", l->w, l->agents, l->counters, counters_dev, mode, exponent, floor, (hipStream_t)stream);
}

int crl_ledger_get_counters(crl_ledger *l, int64_t *counters_out_dev, int64_t *ignored_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counters_out_dev) return crl_fail(CRL_EINVAL, "crl_ledger_get_counters: null argument");
    return books_get_counters(l, counters_out_dev, ignored_out_dev, (hipStream_t)stream);
}

int crl_ledger_set_counters(crl_ledger *l, const int64_t *counters_dev, const int64_t *ignored_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counters_dev) return crl_fail(CRL_EINVAL, "crl_ledger_set_counters: null argument");
    return books_set_counters(l, counters_dev, ignored_dev, (hipStream_t)stream);
}

int crl_ledger_get_env_state(crl_ledger *l, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_get_env_state: null ledger");
    return books_get_env_state(l, ret_out_dev, len_out_dev, draw_ctr_out_dev, (hipStream_t)stream);
}

int crl_ledger_set_env_state(crl_ledger *l, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_ledger_set_env_state: null ledger");
    return books_set_env_state(l, ret_dev, len_dev, draw_ctr_dev, (hipStream_t)stream);
}

int crl_ledger_step(crl_ledger *l, const int32_t *assign_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev,
                    int32_t redraw, int32_t *ids_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !assign_dev || !reward_dev || !done_dev || !ids_out_dev) return crl_fail(CRL_EINVAL, "crl_ledger_step: null argument");
    if (reward_stride < 1) return crl_fail(CRL_EINVAL, "crl_ledger_step: reward_stride must be >= 1 (float32 elements)");
    return books_step<LedgerTraits>(l, assign_dev, reward_dev, reward_stride, done_dev, redraw, ids_out_dev, (hipStream_t)stream);
}

}  // extern "C"

// car_league.hip -- CarRacing's league (include/crl.h "car league"): a pool of opponents for car 1, the per-env weighted draw of who
// drives it, and the books of how car 0 fares against every pool entry.  An object beside a two-car CarRacing context, a
// crl_car_policy and a crl_car_driver of that context: it reads the step's rewards and done flags and writes column 1 of both
// objects' device assignment arrays; nothing here reaches into the step pipeline or serves an action.
//
// Stands in for what a league trainer around make_competitive_car_racing (car_racing/make_competitive_car_racing.py:10-58: ONE
// opponent_policy for the env's life) does on the host: summing both cars' rewards per episode, booking the result under the opponent
// that drove, and handing the env another opponent when it resets.  Here that is one launch per step with one lane per env, in the
// shape of books_step_kernel (pong_books.h): a wavefront without an episode end leaves after its loads and stores; one with some
// books them by the keys present with books_book_wave, the loop of the Pong books.  What differs from the Pong books and makes this a
// kernel of its own: two float32 returns per env, quantised when booked, and the two assignment writes of a redraw.  The table of one
// weight per agent is the ledger's: its draw and its two writers are pong_books.h's.
#include <math.h>

#include "car_device.h"
#include "crl_internal.h"
#include "pong_books.h"

#pragma clang fp contract(off)

namespace crl {

static constexpr int kCLAgents = CRL_LEAGUE_MAX_AGENTS;
static constexpr int kCLPlanes = CRL_CAR_LEAGUE_COUNTERS;
static constexpr int kCLWords = kCLPlanes * kCLAgents;

// the pool as a launch carries it (kernel arguments): what serving entry a writes into column 1 of the two assignment arrays
struct CarLeaguePool {
    int8_t net[kCLAgents];    // the policy's slot, -1 for a style
    int8_t style[kCLAgents];  // the driver's slot, -1 for a network
};

// q of "car league": a return in units of 1/256
__device__ inline long long car_league_q(float x) {
    if (!isfinite(x)) return 0;
    double v = (double)x * 256.0;
    v = v < -0x1p62 ? -0x1p62 : v > 0x1p62 ? 0x1p62 : v;
    return llrint(v);
}

struct CarLeagueArgs {
    int32_t *agent;            // [n]
    float *ret;                // [n][2]
    int32_t *len;              // [n]
    uint32_t *draw_ctr;        // [n]
    unsigned long long *counters;  // [kCLPlanes][kCLAgents]
    const uint32_t *w;         // [kCLAgents]
    int32_t *policy_assign;    // [n][2], the policy's own
    int32_t *driver_assign;    // [n][2], the driver's own
    int64_t n, id_base;
    uint64_t seed;
    int32_t agents;
    CarLeaguePool pool;
};

// serving entry a in env i: column 1 of both arrays (column 0 is the caller's)
__device__ inline void car_league_serve(const CarLeagueArgs &A, int64_t i, int a) {
    A.agent[i] = a;
    A.policy_assign[2 * i + 1] = A.pool.net[a];
    A.driver_assign[2 * i + 1] = A.pool.style[a];
}

// step 3 of "car league" for env i: a table without a draw keeps agent, counter and assignments
__device__ inline void car_league_redraw(const CarLeagueArgs &A, int64_t i) {
    const uint32_t ctr = A.draw_ctr[i];
    const int drawn = books_draw16(A.w, A.seed, (uint64_t)(A.id_base + i), ctr, CRL_CAR_LEAGUE_DOMAIN);
    if (drawn >= 0 && drawn < A.agents) car_league_serve(A, i, drawn), A.draw_ctr[i] = ctr + 1;
}

__global__ __launch_bounds__(kBThreads) void car_league_step_kernel(const CarLeagueArgs A, const float *__restrict__ reward,
                                                                   const uint8_t *__restrict__ done, int redraw) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    int key = -1;  // the entry this lane's finished episode goes to; -1: no episode ended here, or its agent lies outside the pool
    float r0 = 0.f, r1 = 0.f;
    int steps = 0;
    if (i < A.n) {
        r0 = A.ret[2 * i] + reward[2 * i], r1 = A.ret[2 * i + 1] + reward[2 * i + 1];
        steps = A.len[i] + 1;
        const bool d = done[i] != 0;
        if (d) {
            const int a = A.agent[i];
            if (a >= 0 && a < A.agents) key = a;
            if (redraw) car_league_redraw(A, i);
        }
        A.ret[2 * i] = d ? 0.f : r0, A.ret[2 * i + 1] = d ? 0.f : r1, A.len[i] = d ? 0 : steps;
    }
    long long sums[3] = {0ll, 0ll, (long long)steps};  // both returns in units of 1/256, the length
    if (key >= 0) sums[0] = car_league_q(r0), sums[1] = car_league_q(r1);
    books_book_wave(key, r0 > r1, r0 < r1, sums, A.counters, kCLAgents);
}

__global__ __launch_bounds__(kBThreads) void car_league_draw_all_kernel(const CarLeagueArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (i < A.n) car_league_redraw(A, i);
}

// crl_car_league_set_env_state wrote the agent array: serve what it names
__global__ __launch_bounds__(kBThreads) void car_league_apply_kernel(const CarLeagueArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (i >= A.n) return;
    const int a = A.agent[i];
    if (a >= 0 && a < A.agents) car_league_serve(A, i, a);
}

__global__ void car_league_set_weight_kernel(int a, uint32_t value, uint32_t *__restrict__ w) {
    if (threadIdx.x == 0) w[a] = value;
}

__global__ void car_league_reset_agent_kernel(int a, unsigned long long *__restrict__ counters) {
    if (threadIdx.x < kCLPlanes) counters[threadIdx.x * kCLAgents + a] = 0ull;
}

}  // namespace crl

using namespace crl;

struct crl_car_league {
    crl_car_policy *policy = nullptr;
    crl_car_driver *driver = nullptr;
    int64_t n = 0, id_base = 0;
    uint64_t seed = 0;
    int agents = 0;
    int32_t kind[kCLAgents], slot[kCLAgents];
    int32_t *agent = nullptr;               // [n]
    float *ret = nullptr;                   // [n][2]
    int32_t *len = nullptr;                 // [n]
    uint32_t *draw_ctr = nullptr;           // [n]
    unsigned long long *counters = nullptr;  // [kCLPlanes][kCLAgents]
    uint32_t *w = nullptr;                  // [kCLAgents]

    unsigned blocks() const { return (unsigned)((n + kBThreads - 1) / kBThreads); }
};

static CarLeagueArgs car_league_args(const crl_car_league *l) {
    CarLeagueArgs A;
    A.agent = l->agent, A.ret = l->ret, A.len = l->len, A.draw_ctr = l->draw_ctr, A.counters = l->counters, A.w = l->w;
    A.policy_assign = crl_car_policy_assign_dev(l->policy), A.driver_assign = crl_car_driver_assign_dev(l->driver);
    A.n = l->n, A.id_base = l->id_base, A.seed = l->seed, A.agents = l->agents;
    for (int a = 0; a < kCLAgents; a++) {
        const bool in = a < l->agents;
        A.pool.net[a] = (int8_t)(in && l->kind[a] == CRL_CAR_LEAGUE_NETWORK ? l->slot[a] : -1);
        A.pool.style[a] = (int8_t)(in && l->kind[a] == CRL_CAR_LEAGUE_STYLE ? l->slot[a] : -1);
    }
    return A;
}

extern "C" {

void crl_car_league_destroy(crl_car_league *l) {
    if (!l) return;
    if (l->agent) (void)hipFree(l->agent);
    if (l->ret) (void)hipFree(l->ret);
    if (l->len) (void)hipFree(l->len);
    if (l->draw_ctr) (void)hipFree(l->draw_ctr);
    if (l->counters) (void)hipFree(l->counters);
    if (l->w) (void)hipFree(l->w);
    delete l;
}

int crl_car_league_create(crl_ctx *ctx, crl_car_policy *policy, crl_car_driver *driver, uint64_t seed, crl_car_league **out) {
    crl_fail_no_ctx();
    if (!ctx || !policy || !driver || !out) return crl_fail(CRL_EINVAL, "crl_car_league_create: null argument");
    crl_car_ctx *car = crl_ctx_car(ctx);
    if (!car) return crl_fail(CRL_EINVAL, "crl_car_league_create: not a CarRacing context");
    const CarSoA *s = crl_car_soa(car);
    if (s->players != 2) return crl_fail(CRL_EINVAL, "crl_car_league_create: the opponent drives car 1: a two-car context is needed, not one of %d car", s->players);
    if (crl_car_policy_ctx(policy) != car || crl_car_driver_ctx(driver) != car)
        return crl_fail(CRL_EINVAL, "crl_car_league_create: the policy and the driver must belong to this context");
    const char *what = "crl_car_league_create";
    crl_car_league *l = new crl_car_league();
    l->policy = policy, l->driver = driver, l->n = s->n, l->id_base = crl_car_env_id_base(car), l->seed = seed;
    for (int a = 0; a < kCLAgents; a++) l->kind[a] = l->slot[a] = -1;
    const size_t n = (size_t)l->n;
    int rc = crl_dev_zalloc(&l->agent, n * sizeof(int32_t), what);
    if (!rc) rc = crl_dev_zalloc(&l->ret, n * 2 * sizeof(float), what);
    if (!rc) rc = crl_dev_zalloc(&l->len, n * sizeof(int32_t), what);
    if (!rc) rc = crl_dev_zalloc(&l->draw_ctr, n * sizeof(uint32_t), what);
    if (!rc) rc = crl_dev_zalloc(&l->counters, kCLWords * sizeof(unsigned long long), what);
    if (!rc) rc = crl_dev_zalloc(&l->w, kCLAgents * sizeof(uint32_t), what);
    if (!rc) {
        const hipError_t e = hipMemset(l->agent, 0xFF, n * sizeof(int32_t));  // -1: no draw yet
        if (e != hipSuccess) rc = crl_hip_fail(e, what);
    }
    if (rc) {
        crl_car_league_destroy(l);
        return rc;
    }
    *out = l;
    return CRL_OK;
}

int crl_car_league_add_agent(crl_car_league *l, int32_t kind, int32_t slot, int32_t *id_out, void *stream) {
    crl_fail_no_ctx();
    if (kind != CRL_CAR_LEAGUE_NETWORK && kind != CRL_CAR_LEAGUE_STYLE)
        return crl_fail(CRL_EINVAL, "crl_car_league_add_agent: kind must be CRL_CAR_LEAGUE_NETWORK or CRL_CAR_LEAGUE_STYLE, not %d", kind);
    const int slots = kind == CRL_CAR_LEAGUE_NETWORK ? CRL_CAR_POLICY_SLOTS : CRL_CAR_DRIVER_SLOTS;
    if (slot < 0 || slot >= slots) return crl_fail(CRL_EINVAL, "crl_car_league_add_agent: slot %d lies outside [0, %d)", slot, slots);
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_add_agent: null league");
    if (l->agents >= kCLAgents) return crl_fail(CRL_EINVAL, "crl_car_league_add_agent: the pool holds %d agents already", kCLAgents);
    hipLaunchKernelGGL(car_league_set_weight_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, l->agents, 1u, l->w);
    HIP_TRY(hipGetLastError());
    l->kind[l->agents] = kind, l->slot[l->agents] = slot;
    if (id_out) *id_out = l->agents;
    l->agents++;
    return CRL_OK;
}

int crl_car_league_get_pool(crl_car_league *l, int32_t *agents_out, int32_t *kinds_out, int32_t *slots_out) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_get_pool: null league");
    if (agents_out) *agents_out = l->agents;
    for (int a = 0; a < kCLAgents; a++) {
        if (kinds_out) kinds_out[a] = l->kind[a];
        if (slots_out) slots_out[a] = l->slot[a];
    }
    return CRL_OK;
}

int crl_car_league_draw_all(crl_car_league *l, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_draw_all: null league");
    hipLaunchKernelGGL(car_league_draw_all_kernel, dim3(l->blocks()), dim3(kBThreads), 0, (hipStream_t)stream, car_league_args(l));
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_car_league_seed(crl_car_league *l, uint64_t seed, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_seed: null league");
    HIP_TRY(hipMemsetAsync(l->draw_ctr, 0, (size_t)l->n * sizeof(uint32_t), (hipStream_t)stream));
    l->seed = seed;
    return CRL_OK;
}

int crl_car_league_reset(crl_car_league *l, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_reset: null league");
    HIP_TRY(hipMemsetAsync(l->counters, 0, kCLWords * sizeof(unsigned long long), (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(l->ret, 0, (size_t)l->n * 2 * sizeof(float), (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(l->len, 0, (size_t)l->n * sizeof(int32_t), (hipStream_t)stream));
    return CRL_OK;
}

int crl_car_league_reset_agent(crl_car_league *l, int32_t agent, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_reset_agent: null league");
    if (agent < 0 || agent >= l->agents) return crl_fail(CRL_EINVAL, "crl_car_league_reset_agent: agent %d lies outside the pool of %d", agent, l->agents);
    hipLaunchKernelGGL(car_league_reset_agent_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, agent, l->counters);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_car_league_set_weights(crl_car_league *l, const uint32_t *w_host, int32_t count, void *stream) {
    crl_fail_no_ctx();
    if (!l || !w_host) return crl_fail(CRL_EINVAL, "crl_car_league_set_weights: null argument");
    return books_set_weights16("crl_car_league_set_weights", l->w, l->agents, w_host, count, (hipStream_t)stream);
}

int crl_car_league_get_weights(crl_car_league *l, uint32_t *w_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !w_out_dev) return crl_fail(CRL_EINVAL, "crl_car_league_get_weights: null argument");
    return books_copy(w_out_dev, l->w, kCLAgents * sizeof(uint32_t), (hipStream_t)stream);
}

int crl_car_league_pfsp_weights(crl_car_league *l, const int64_t *counters_dev, int32_t mode, int32_t exponent, uint32_t floor, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_pfsp_weights: null league");
    return books_pfsp16("crl_car_league_pfsp_weights", l->w, l->agents, l->counters, counters_dev, mode, exponent, floor, (hipStream_t)stream);
}

int crl_car_league_get_counters(crl_car_league *l, int64_t *counters_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counters_out_dev) return crl_fail(CRL_EINVAL, "crl_car_league_get_counters: null argument");
    return books_copy(counters_out_dev, l->counters, kCLWords * sizeof(int64_t), (hipStream_t)stream);
}

int crl_car_league_set_counters(crl_car_league *l, const int64_t *counters_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counters_dev) return crl_fail(CRL_EINVAL, "crl_car_league_set_counters: null argument");
    return books_copy(l->counters, counters_dev, kCLWords * sizeof(int64_t), (hipStream_t)stream);
}

int crl_car_league_get_env_state(crl_car_league *l, int32_t *agent_out_dev, float *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev,
                                 void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_get_env_state: null league");
    const size_t bytes = (size_t)l->n * sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    int rc = books_copy(agent_out_dev, l->agent, bytes, st);
    if (rc == CRL_OK) rc = books_copy(ret_out_dev, l->ret, 2 * bytes, st);
    if (rc == CRL_OK) rc = books_copy(len_out_dev, l->len, bytes, st);
    return rc != CRL_OK ? rc : books_copy(draw_ctr_out_dev, l->draw_ctr, bytes, st);
}

int crl_car_league_set_env_state(crl_car_league *l, const int32_t *agent_dev, const float *ret_dev, const int32_t *len_dev,
                                 const uint32_t *draw_ctr_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_car_league_set_env_state: null league");
    const size_t bytes = (size_t)l->n * sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    int rc = books_copy(l->agent, agent_dev, bytes, st);
    if (rc == CRL_OK) rc = books_copy(l->ret, ret_dev, 2 * bytes, st);
    if (rc == CRL_OK) rc = books_copy(l->len, len_dev, bytes, st);
    if (rc == CRL_OK) rc = books_copy(l->draw_ctr, draw_ctr_dev, bytes, st);
    if (rc != CRL_OK || !agent_dev) return rc;
    hipLaunchKernelGGL(car_league_apply_kernel, dim3(l->blocks()), dim3(kBThreads), 0, st, car_league_args(l));
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_car_league_get_assignment(crl_car_league *l, int32_t *agent_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !agent_out_dev) return crl_fail(CRL_EINVAL, "crl_car_league_get_assignment: null argument");
    return books_copy(agent_out_dev, l->agent, (size_t)l->n * sizeof(int32_t), (hipStream_t)stream);
}

int crl_car_league_step(crl_car_league *l, const float *rewards_dev, const uint8_t *done_dev, int32_t redraw, void *stream) {
    crl_fail_no_ctx();
    if (!l || !rewards_dev || !done_dev) return crl_fail(CRL_EINVAL, "crl_car_league_step: null argument");
    hipLaunchKernelGGL(car_league_step_kernel, dim3(l->blocks()), dim3(kBThreads), 0, (hipStream_t)stream, car_league_args(l), rewards_dev, done_dev,
                       (int)(redraw != 0));
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

}  // extern "C"

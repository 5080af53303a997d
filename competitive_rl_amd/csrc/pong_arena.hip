// pong_arena.hip -- the pool-vs-pool arena: how every agent of a pool fares against every other, booked per (left, right) pair, and
// the draw of an env's next pair (include/crl.h "arena books", "arena draws", "balance weights").  An object beside crl_league, as
// crl_ledger is: nothing here reaches into a league, the caller passes the pairs in and takes the next pairs out.
//
// Stands in for the reference's evaluate_two_policies_in_batch (pong/evaluate.py:6-88), which plays ONE pair of policies with the
// host walking every step, called once per pair of a pool: here one batch holds the whole round-robin, one launch per step with one
// lane per env, books_step_kernel of pong_books.h keyed by the cell left * 16 + right.  This file holds what knows that key: the draw
// over the row sums and the row, the kernels that write the table (the balance rule among them) and the entry points; lifetime, seed,
// reset and the copies are the shared Books'.
#include "pong_books.h"

namespace crl {

static constexpr int kAAgents = kBAgents;
static constexpr int kACells = kAAgents * kAAgents;    // 256, cell = left * 16 + right
static constexpr int kACounters = kBPlanes * kACells;  // int64 words; `ignored` is word kACounters
static constexpr int kATable = kACells + kAAgents;     // uint32 words: w[256], then the 16 row sums the draw walks first

struct ArenaTable {
    uint32_t w[kACells];
};

struct ArenaTraits {
    static constexpr int kIds = 2, kKeys = kACells;
    static __device__ int key(const int32_t *ids, int agents) {
        return (ids[0] >= 0 && ids[0] < agents && ids[1] >= 0 && ids[1] < agents) ? ids[0] * kAAgents + ids[1] : -2;
    }
    // include/crl.h "arena draws": the smallest row-major cell whose cumulative weight exceeds (x0 * T) >> 32, found over the 16 row sums
    // and then inside the row; -1 when the table sums to 0 (or past 2^32)
    static __device__ int draw(const uint32_t *__restrict__ w, uint64_t seed, uint64_t gid, uint32_t n) {
        const uint32_t *rows = w + kACells;
        uint64_t total = 0;
#pragma unroll
        for (int a = 0; a < kAAgents; a++) total += rows[a];
        if (total - 1 >= 0xFFFFFFFFull) return -1;
        const uint64_t r = league_draw(seed, gid, n, CRL_ARENA_DOMAIN_PAIR, (uint32_t)total);
        uint64_t cum = 0, before = 0;
        int row = -1;
#pragma unroll
        for (int a = 0; a < kAAgents; a++) {
            if (row < 0 && cum + rows[a] > r) row = a, before = cum;
            cum += rows[a];
        }
        if (row < 0) return -1;  // (not reached: cum ends at total > r)
        const uint32_t *wr = w + row * kAAgents;
        cum = before;
        int col = -1;
#pragma unroll
        for (int b = 0; b < kAAgents; b++) {
            cum += wr[b];
            if (col < 0 && cum > r) col = b;
        }
        return col < 0 ? -1 : row * kAAgents + col;
    }
    static __device__ void put(int key, int32_t *ids) { ids[0] = key / kAAgents, ids[1] = key % kAAgents; }
};

// a fresh arena draw for every env (a table that sums to 0 keeps the pair and the counter)
__global__ __launch_bounds__(kBThreads) void arena_draw_kernel(const int32_t *pairs, uint32_t *__restrict__ draw_ctr, const uint32_t *__restrict__ w,
                                                              uint64_t seed, int64_t env_id_base, int64_t n, int32_t *pairs_out) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    if (i >= n) return;
    int32_t ids[2] = {pairs[2 * i], pairs[2 * i + 1]};
    books_redraw<ArenaTraits>(ids, draw_ctr + i, w, seed, (uint64_t)(env_id_base + i));
    pairs_out[2 * i] = ids[0], pairs_out[2 * i + 1] = ids[1];
}

// The tail of every kernel that writes the table (one workgroup, lane = cell): the cell's weight and the 16 row sums.
__device__ inline void arena_store_table(uint32_t mine, uint32_t *__restrict__ w, uint32_t *lds) {
    const int c = threadIdx.x;
    lds[c] = mine;
    w[c] = mine;
    __syncthreads();
    if (c < kAAgents) {
        uint32_t s = 0;
#pragma unroll
        for (int b = 0; b < kAAgents; b++) s += lds[c * kAAgents + b];
        w[kACells + c] = s;
    }
}

// include/crl.h "balance weights": one workgroup, lane = cell; integers only
__global__ __launch_bounds__(kACells) void arena_balance_kernel(const long long *__restrict__ counters, int agents, int include_mirror, uint32_t floor_w,
                                                               uint32_t *__restrict__ w) {
    __shared__ long long top[kACells];
    __shared__ uint32_t table[kACells];
    const int c = threadIdx.x, left = c / kAAgents, right = c % kAAgents;
    const bool scheduled = left < agents && right < agents && (include_mirror || left != right);
    const long long e = counters[CRL_ARENA_EPISODES * kACells + c];
    top[c] = scheduled ? e : (long long)0x8000000000000000ull;
    __syncthreads();
    for (int s = kACells / 2; s >= 1; s >>= 1) {
        if (c < s && top[c + s] > top[c]) top[c] = top[c + s];
        __syncthreads();
    }
    uint32_t out = 0;
    if (scheduled) {
        const unsigned long long behind = (unsigned long long)top[0] - (unsigned long long)e;
        out = floor_w + (uint32_t)(behind < 65535ull ? behind : 65535ull);
    }
    arena_store_table(out, w, table);
}

__global__ __launch_bounds__(kACells) void arena_set_weights_kernel(ArenaTable t, uint32_t *__restrict__ w) {
    __shared__ uint32_t table[kACells];
    arena_store_table(t.w[threadIdx.x], w, table);
}

// cells that enter the pool get weight 1 off the diagonal (0 on it), cells that leave it weight 0
__global__ __launch_bounds__(kACells) void arena_resize_kernel(int before, int after, uint32_t *__restrict__ w) {
    __shared__ uint32_t table[kACells];
    const int c = threadIdx.x, left = c / kAAgents, right = c % kAAgents;
    uint32_t mine = w[c];
    if (left >= after || right >= after) mine = 0;
    else if (left >= before || right >= before) mine = left != right ? 1u : 0u;
    arena_store_table(mine, w, table);
}

}  // namespace crl

using namespace crl;

struct crl_arena : Books {};  // counters [CRL_ARENA_COUNTERS][kACells], then `ignored`; w [kACells], then the row sums [kAAgents]

extern "C" {

int crl_arena_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int32_t agents, crl_arena **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || num_envs > 0x3fffffff || env_id_base < 0 || agents < 1 || agents > kAAgents)
        return crl_fail(CRL_EINVAL, "crl_arena_create: bad arguments (num_envs in [1, 2^30), env_id_base >= 0, agents in [1, %d])", kAAgents);
    return books_create("crl_arena_create", device, num_envs, env_id_base, seed, agents, kACounters, kATable,
                        [](uint32_t *w, int pool) { hipLaunchKernelGGL(arena_resize_kernel, dim3(1), dim3(kACells), 0, nullptr, 0, pool, w); }, out);
}

void crl_arena_destroy(crl_arena *a) { books_destroy(a); }

int crl_arena_seed(crl_arena *a, uint64_t seed, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_seed: null arena");
    return books_seed(a, seed, (hipStream_t)stream);
}

int crl_arena_reset(crl_arena *a, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_reset: null arena");
    return books_reset(a, (hipStream_t)stream);
}

int crl_arena_set_agents(crl_arena *a, int32_t agents, void *stream) {
    crl_fail_no_ctx();
    if (!a || agents < 1 || agents > kAAgents) return crl_fail(CRL_EINVAL, "crl_arena_set_agents: agents must be in [1, %d]", kAAgents);
    hipLaunchKernelGGL(arena_resize_kernel, dim3(1), dim3(kACells), 0, (hipStream_t)stream, a->agents, agents, a->w);
    HIP_TRY(hipGetLastError());
    a->agents = agents;
    return CRL_OK;
}

int crl_arena_set_weights(crl_arena *a, const uint32_t *w_host, int32_t count, void *stream) {
    crl_fail_no_ctx();
    if (!a || !w_host) return crl_fail(CRL_EINVAL, "crl_arena_set_weights: null argument");
    if (count != a->agents * a->agents)
        return crl_fail(CRL_EINVAL, "crl_arena_set_weights: %d weights for a pool of %d agents (%d cells)", count, a->agents, a->agents * a->agents);
    ArenaTable t{};
    uint64_t total = 0;
    for (int l = 0; l < a->agents; l++)
        for (int r = 0; r < a->agents; r++) t.w[l * kAAgents + r] = w_host[l * a->agents + r], total += w_host[l * a->agents + r];
    if (total == 0 || total >= (1ull << 32))
        return crl_fail(CRL_EINVAL, "crl_arena_set_weights: the weights must sum to a value in [1, 2^32), not %llu", (unsigned long long)total);
    hipLaunchKernelGGL(arena_set_weights_kernel, dim3(1), dim3(kACells), 0, (hipStream_t)stream, t, a->w);  // (the table travels as kernel arguments)
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_arena_get_weights(crl_arena *a, uint32_t *w_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !w_out_dev) return crl_fail(CRL_EINVAL, "crl_arena_get_weights: null argument");
    return books_get_weights(a, w_out_dev, kACells, (hipStream_t)stream);
}

int crl_arena_balance_weights(crl_arena *a, const int64_t *counters_dev, int32_t include_mirror, uint32_t floor, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_balance_weights: null arena");
    if ((uint64_t)a->agents * (uint64_t)a->agents * ((uint64_t)floor + 65535u) >= (1ull << 32))
        return crl_fail(CRL_EINVAL, "crl_arena_balance_weights: floor %u lets the weights of %d x %d cells sum past 2^32", floor, a->agents, a->agents);
    const long long *src = counters_dev ? reinterpret_cast<const long long *>(counters_dev) : reinterpret_cast<const long long *>(a->counters);
    hipLaunchKernelGGL(arena_balance_kernel, dim3(1), dim3(kACells), 0, (hipStream_t)stream, src, a->agents, include_mirror != 0, floor, a->w);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_arena_get_counters(crl_arena *a, int64_t *counters_out_dev, int64_t *ignored_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !counters_out_dev) return crl_fail(CRL_EINVAL, "crl_arena_get_counters: null argument");
    return books_get_counters(a, counters_out_dev, ignored_out_dev, (hipStream_t)stream);
}

int crl_arena_set_counters(crl_arena *a, const int64_t *counters_dev, const int64_t *ignored_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !counters_dev) return crl_fail(CRL_EINVAL, "crl_arena_set_counters: null argument");
    return books_set_counters(a, counters_dev, ignored_dev, (hipStream_t)stream);
}

int crl_arena_get_env_state(crl_arena *a, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_get_env_state: null arena");
    return books_get_env_state(a, ret_out_dev, len_out_dev, draw_ctr_out_dev, (hipStream_t)stream);
}

int crl_arena_set_env_state(crl_arena *a, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_set_env_state: null arena");
    return books_set_env_state(a, ret_dev, len_dev, draw_ctr_dev, (hipStream_t)stream);
}

int crl_arena_draw(crl_arena *a, const int32_t *pairs_dev, int32_t *pairs_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !pairs_dev || !pairs_out_dev) return crl_fail(CRL_EINVAL, "crl_arena_draw: null argument");
    hipLaunchKernelGGL(arena_draw_kernel, dim3(a->blocks()), dim3(kBThreads), 0, (hipStream_t)stream, pairs_dev, a->draw_ctr, a->w, a->seed,
                       a->env_id_base, a->n, pairs_out_dev);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_arena_step(crl_arena *a, const int32_t *pairs_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev, int32_t redraw,
                   int32_t *pairs_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !pairs_dev || !reward_dev || !done_dev || !pairs_out_dev) return crl_fail(CRL_EINVAL, "crl_arena_step: null argument");
    if (reward_stride < 1) return crl_fail(CRL_EINVAL, "crl_arena_step: reward_stride must be >= 1 (float32 elements)");
    return books_step<ArenaTraits>(a, pairs_dev, reward_dev, reward_stride, done_dev, redraw, pairs_out_dev, (hipStream_t)stream);
}

}  // extern "C"

// pong_arena.hip -- the pool-vs-pool arena: how every agent of a pool fares against every other, booked per (left, right) pair, and
// the draw of an env's next pair (include/crl.h "arena books", "arena draws", "balance weights").  An object beside crl_league, as
// crl_ledger is: nothing here reaches into a league, the caller passes the pairs in and takes the next pairs out.
//
// Stands in for the reference's evaluate_two_policies_in_batch (pong/evaluate.py:6-88), which plays ONE pair of policies with the
// host walking every step, called once per pair of a pool: here one batch holds the whole round-robin, one launch per step with one
// lane per env.  Episode ends are rare, so a wavefront without one leaves after its loads and stores; one with some reduces them by
// the cells actually present (the first remaining lane's cell, a ballot of the lanes on it, popcounts and a shuffle tree for the two
// sums) and the cell's first lane adds with six 64-bit atomics.  Integer sums: the totals do not depend on arrival order.
#include "crl_internal.h"
#include "pong_device.h"

namespace crl {

static constexpr int kAThreads = 256;
static constexpr int kAAgents = CRL_LEAGUE_MAX_AGENTS;
static constexpr int kACells = kAAgents * kAAgents;              // 256, cell = left * 16 + right
static constexpr int kACounters = CRL_ARENA_COUNTERS * kACells;  // int64 words; `ignored` is word kACounters
static constexpr int kATable = kACells + kAAgents;               // uint32 words: w[256], then the 16 row sums the draw walks first

struct ArenaTable {
    uint32_t w[kACells];
};

__device__ inline long long arena_wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// include/crl.h "arena draws": the smallest row-major cell whose cumulative weight exceeds (x0 * T) >> 32, found over the 16 row sums
// and then inside the row; -1 when the table sums to 0 (or past 2^32)
__device__ inline int arena_draw(const uint32_t *__restrict__ w, uint64_t seed, uint64_t gid, uint32_t n) {
    const uint32_t *rows = w + kACells;
    uint64_t total = 0;
#pragma unroll
    for (int a = 0; a < kAAgents; a++) total += rows[a];
    if (total - 1 >= 0xFFFFFFFFull) return -1;
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), n, CRL_ARENA_DOMAIN_PAIR};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t r = ((uint64_t)c[0] * total) >> 32;
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

__global__ __launch_bounds__(kAThreads) void arena_step_kernel(int agents, const int32_t *pairs, const float *__restrict__ reward, int64_t reward_stride,
                                                              const uint8_t *__restrict__ done, int redraw, int32_t *__restrict__ ret,
                                                              int32_t *__restrict__ len, uint32_t *__restrict__ draw_ctr,
                                                              unsigned long long *__restrict__ counters, const uint32_t *__restrict__ w, uint64_t seed,
                                                              int64_t env_id_base, int64_t n, int32_t *pairs_out) {
    const int64_t i = (int64_t)blockIdx.x * kAThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int cell = -1;  // the cell this lane's finished episode goes to; -2: an id outside the pool; -1: no episode ended here
    int r = 0, steps = 0;
    if (i < n) {
        int left = pairs[2 * i], right = pairs[2 * i + 1];
        r = ret[i] + (int)reward[i * reward_stride];
        steps = len[i] + 1;
        const bool d = done[i] != 0;
        if (d) {
            cell = (left >= 0 && left < agents && right >= 0 && right < agents) ? left * kAAgents + right : -2;
            if (redraw) {
                const uint32_t ctr = draw_ctr[i];
                const int drawn = arena_draw(w, seed, (uint64_t)(env_id_base + i), ctr);
                if (drawn >= 0) left = drawn / kAAgents, right = drawn % kAAgents, draw_ctr[i] = ctr + 1;
            }
        }
        ret[i] = d ? 0 : r, len[i] = d ? 0 : steps;
        pairs_out[2 * i] = left, pairs_out[2 * i + 1] = right;
    }
    if (!__ballot(cell != -1)) return;  // (uniform) the usual case: no episode of this wavefront ended
    unsigned long long rest = __ballot(cell >= 0);
    while (rest) {  // (uniform) one round per cell present in this wavefront
        const int c = __shfl(cell, __ffsll(rest) - 1);
        const bool mine = cell == c;
        const unsigned long long m = __ballot(mine);
        const unsigned long long won = __ballot(mine && r > 0), lost = __ballot(mine && r < 0);
        const long long ret_sum = arena_wave_sum(mine ? (long long)r : 0ll), len_sum = arena_wave_sum(mine ? (long long)steps : 0ll);
        if (lane == __ffsll(m) - 1) {
            const unsigned long long e = (unsigned long long)__popcll(m), nl = (unsigned long long)__popcll(won), nr = (unsigned long long)__popcll(lost);
            atomicAdd(&counters[CRL_ARENA_EPISODES * kACells + c], e);
            if (nl) atomicAdd(&counters[CRL_ARENA_LEFT_WINS * kACells + c], nl);
            if (nr) atomicAdd(&counters[CRL_ARENA_RIGHT_WINS * kACells + c], nr);
            if (e - nl - nr) atomicAdd(&counters[CRL_ARENA_DRAWS * kACells + c], e - nl - nr);
            atomicAdd(&counters[CRL_ARENA_RETURN_SUM * kACells + c], (unsigned long long)ret_sum);
            atomicAdd(&counters[CRL_ARENA_LENGTH_SUM * kACells + c], (unsigned long long)len_sum);
        }
        rest &= ~m;
    }
    const unsigned long long stray = __ballot(cell == -2);
    if (stray && lane == __ffsll(stray) - 1) atomicAdd(&counters[kACounters], (unsigned long long)__popcll(stray));
}

// a fresh arena draw for every env (a table that sums to 0 keeps the pair and the counter)
__global__ __launch_bounds__(kAThreads) void arena_draw_kernel(const int32_t *pairs, uint32_t *__restrict__ draw_ctr, const uint32_t *__restrict__ w,
                                                              uint64_t seed, int64_t env_id_base, int64_t n, int32_t *pairs_out) {
    const int64_t i = (int64_t)blockIdx.x * kAThreads + threadIdx.x;
    if (i >= n) return;
    int left = pairs[2 * i], right = pairs[2 * i + 1];
    const uint32_t ctr = draw_ctr[i];
    const int drawn = arena_draw(w, seed, (uint64_t)(env_id_base + i), ctr);
    if (drawn >= 0) left = drawn / kAAgents, right = drawn % kAAgents, draw_ctr[i] = ctr + 1;
    pairs_out[2 * i] = left, pairs_out[2 * i + 1] = right;
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

struct crl_arena {
    int device = 0;
    int64_t n = 0, env_id_base = 0;
    uint64_t seed = 0;
    int agents = 0;
    int32_t *ret = nullptr, *len = nullptr;
    uint32_t *draw_ctr = nullptr;
    unsigned long long *counters = nullptr;  // [CRL_ARENA_COUNTERS][kACells], then `ignored`
    uint32_t *w = nullptr;                   // [kACells], then the row sums [kAAgents]
};

static int arena_copy(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (dst && src) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return CRL_OK;
}

static unsigned arena_blocks(const crl_arena *a) { return (unsigned)((a->n + kAThreads - 1) / kAThreads); }

extern "C" {

int crl_arena_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int32_t agents, crl_arena **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || num_envs > 0x3fffffff || env_id_base < 0 || agents < 1 || agents > kAAgents)
        return crl_fail(CRL_EINVAL, "crl_arena_create: bad arguments (num_envs in [1, 2^30), env_id_base >= 0, agents in [1, %d])", kAAgents);
    HIP_TRY(hipSetDevice(device));
    crl_arena *a = new crl_arena();
    a->device = device, a->n = num_envs, a->env_id_base = env_id_base, a->seed = seed, a->agents = agents;
    const size_t per_env = (size_t)num_envs * sizeof(int32_t), books = (kACounters + 1) * sizeof(unsigned long long);
    const char *what = "crl_arena_create";
    int rc = crl_dev_zalloc(&a->ret, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&a->len, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&a->draw_ctr, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&a->counters, books, what);
    if (!rc) rc = crl_dev_zalloc(&a->w, kATable * sizeof(uint32_t), what);
    if (!rc) {
        hipLaunchKernelGGL(arena_resize_kernel, dim3(1), dim3(kACells), 0, nullptr, 0, agents, a->w);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = crl_hip_fail(e, what);
    }
    if (rc) {
        crl_arena_destroy(a);
        return rc;
    }
    *out = a;
    return CRL_OK;
}

void crl_arena_destroy(crl_arena *a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (a->ret) (void)hipFree(a->ret);
    if (a->len) (void)hipFree(a->len);
    if (a->draw_ctr) (void)hipFree(a->draw_ctr);
    if (a->counters) (void)hipFree(a->counters);
    if (a->w) (void)hipFree(a->w);
    delete a;
}

int crl_arena_seed(crl_arena *a, uint64_t seed, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_seed: null arena");
    HIP_TRY(hipMemsetAsync(a->draw_ctr, 0, (size_t)a->n * sizeof(uint32_t), (hipStream_t)stream));
    a->seed = seed;
    return CRL_OK;
}

int crl_arena_reset(crl_arena *a, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_reset: null arena");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(a->counters, 0, (kACounters + 1) * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(a->ret, 0, (size_t)a->n * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(a->len, 0, (size_t)a->n * sizeof(int32_t), st));
    return CRL_OK;
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
    return arena_copy(w_out_dev, a->w, kACells * sizeof(uint32_t), (hipStream_t)stream);
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
    int rc = arena_copy(counters_out_dev, a->counters, kACounters * sizeof(int64_t), (hipStream_t)stream);
    return rc != CRL_OK ? rc : arena_copy(ignored_out_dev, a->counters + kACounters, sizeof(int64_t), (hipStream_t)stream);
}

int crl_arena_set_counters(crl_arena *a, const int64_t *counters_dev, const int64_t *ignored_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !counters_dev) return crl_fail(CRL_EINVAL, "crl_arena_set_counters: null argument");
    int rc = arena_copy(a->counters, counters_dev, kACounters * sizeof(int64_t), (hipStream_t)stream);
    return rc != CRL_OK ? rc : arena_copy(a->counters + kACounters, ignored_dev, sizeof(int64_t), (hipStream_t)stream);
}

int crl_arena_get_env_state(crl_arena *a, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_get_env_state: null arena");
    const size_t bytes = (size_t)a->n * sizeof(int32_t);
    int rc = arena_copy(ret_out_dev, a->ret, bytes, (hipStream_t)stream);
    if (rc == CRL_OK) rc = arena_copy(len_out_dev, a->len, bytes, (hipStream_t)stream);
    return rc != CRL_OK ? rc : arena_copy(draw_ctr_out_dev, a->draw_ctr, bytes, (hipStream_t)stream);
}

int crl_arena_set_env_state(crl_arena *a, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a) return crl_fail(CRL_EINVAL, "crl_arena_set_env_state: null arena");
    const size_t bytes = (size_t)a->n * sizeof(int32_t);
    int rc = arena_copy(a->ret, ret_dev, bytes, (hipStream_t)stream);
    if (rc == CRL_OK) rc = arena_copy(a->len, len_dev, bytes, (hipStream_t)stream);
    return rc != CRL_OK ? rc : arena_copy(a->draw_ctr, draw_ctr_dev, bytes, (hipStream_t)stream);
}

int crl_arena_draw(crl_arena *a, const int32_t *pairs_dev, int32_t *pairs_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !pairs_dev || !pairs_out_dev) return crl_fail(CRL_EINVAL, "crl_arena_draw: null argument");
    hipLaunchKernelGGL(arena_draw_kernel, dim3(arena_blocks(a)), dim3(kAThreads), 0, (hipStream_t)stream, pairs_dev, a->draw_ctr, a->w, a->seed,
                       a->env_id_base, a->n, pairs_out_dev);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

int crl_arena_step(crl_arena *a, const int32_t *pairs_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev, int32_t redraw,
                   int32_t *pairs_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!a || !pairs_dev || !reward_dev || !done_dev || !pairs_out_dev) return crl_fail(CRL_EINVAL, "crl_arena_step: null argument");
    if (reward_stride < 1) return crl_fail(CRL_EINVAL, "crl_arena_step: reward_stride must be >= 1 (float32 elements)");
    hipLaunchKernelGGL(arena_step_kernel, dim3(arena_blocks(a)), dim3(kAThreads), 0, (hipStream_t)stream, a->agents, pairs_dev, reward_dev,
                       reward_stride, done_dev, redraw, a->ret, a->len, a->draw_ctr, a->counters, a->w, a->seed, a->env_id_base, a->n, pairs_out_dev);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

}  // extern "C"

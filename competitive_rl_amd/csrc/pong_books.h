// pong_books.h -- what the league's two sets of books share: crl_ledger (pong_ledger.hip, keyed by the opponent's id) and crl_arena
// (pong_arena.hip, keyed by the cell left * 16 + right) are the same object with another key.  Here: the step kernel that books a
// batch's finished episodes and redraws their ids, and the host object with everything that does not look at the key (lifetime, seed,
// reset, the copies of counters and per-env state).  What knows the key is a traits type of the including file:
//
//   struct Traits {
//       static constexpr int kIds;    // int32 ids an env carries (1: the opponent; 2: left, right)
//       static constexpr int kKeys;   // width of a counter plane (16 agents; 256 cells)
//       static __device__ int key(const int32_t *ids, int agents);                           // the ids' key; -2: an id outside the pool
//       static __device__ int draw(const uint32_t *w, uint64_t seed, uint64_t gid, uint32_t n);  // a key drawn over the table; -1: no draw
//       static __device__ void put(int key, int32_t *ids);                                   // the ids of a drawn key
//   };
//
// Beside them, what every table of one weight per agent shares (the ledger's, and the CarRacing league's of car_league.hip, which keeps
// its own per-env state): the draw over 16 weights, the table's two writers (pong_ledger.hip) and the booking of a wavefront's finished
// episodes, books_book_wave, which is the loop of both step kernels.
//
// The counter planes have one order in both (include/crl.h crl_ledger_counter / crl_arena_counter): episodes, wins of the first
// party (the learner; the left agent), wins of the second, draws, return sum, length sum; word kBPlanes * kKeys is `ignored`.
#pragma once
#include "crl_internal.h"
#include "pong_device.h"

namespace crl {

static constexpr int kBThreads = 256;
static constexpr int kBAgents = CRL_LEAGUE_MAX_AGENTS;
enum { kBEpisodes = 0, kBWins = 1, kBLosses = 2, kBDraws = 3, kBReturnSum = 4, kBLengthSum = 5, kBPlanes = 6 };
static_assert(CRL_LEDGER_EPISODES == kBEpisodes && CRL_LEDGER_WINS == kBWins && CRL_LEDGER_LOSSES == kBLosses && CRL_LEDGER_DRAWS == kBDraws &&
                  CRL_LEDGER_RETURN_SUM == kBReturnSum && CRL_LEDGER_LENGTH_SUM == kBLengthSum && CRL_LEDGER_COUNTERS == kBPlanes,
              "the ledger's counter planes");
static_assert(CRL_ARENA_EPISODES == kBEpisodes && CRL_ARENA_LEFT_WINS == kBWins && CRL_ARENA_RIGHT_WINS == kBLosses && CRL_ARENA_DRAWS == kBDraws &&
                  CRL_ARENA_RETURN_SUM == kBReturnSum && CRL_ARENA_LENGTH_SUM == kBLengthSum && CRL_ARENA_COUNTERS == kBPlanes,
              "the arena's counter planes");
// the CarRacing league books a third sum: its planes from kBReturnSum on are books_book_wave's sums[0 .. 2]
static_assert(CRL_CAR_LEAGUE_EPISODES == kBEpisodes && CRL_CAR_LEAGUE_WINS == kBWins && CRL_CAR_LEAGUE_LOSSES == kBLosses && CRL_CAR_LEAGUE_DRAWS == kBDraws &&
                  CRL_CAR_LEAGUE_RETURN_SUM == kBReturnSum && CRL_CAR_LEAGUE_RETURN_SUM == 4 && CRL_CAR_LEAGUE_OPPONENT_RETURN_SUM == kBReturnSum + 1 &&
                  CRL_CAR_LEAGUE_LENGTH_SUM == kBReturnSum + 2 && CRL_CAR_LEAGUE_COUNTERS == kBReturnSum + 3,
              "the car league's counter planes");

__device__ inline long long wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// include/crl.h "ledger draws" over a table of one weight per agent: the smallest a whose cumulative weight exceeds (x0 * T) >> 32, x0
// drawn under `domain`; -1 when the table sums to 0 (or past 2^32 - 1)
__device__ inline int books_draw16(const uint32_t *__restrict__ w, uint64_t seed, uint64_t gid, uint32_t n, uint32_t domain) {
    uint64_t total = 0;
#pragma unroll
    for (int a = 0; a < kBAgents; a++) total += w[a];
    if (total - 1 >= 0xFFFFFFFFull) return -1;
    const uint64_t r = league_draw(seed, gid, n, domain, (uint32_t)total);
    uint64_t cum = 0;
    int drawn = -1;
#pragma unroll
    for (int a = 0; a < kBAgents; a++) {
        cum += w[a];
        if (drawn < 0 && cum > r) drawn = a;
    }
    return drawn;
}

// Books a wavefront's finished episodes, all lanes of the wavefront together: `key` >= 0 where this lane's episode ended and goes to
// that key, `won` / `lost` its result, `sums` what it adds to the planes kBReturnSum .. kBReturnSum + NSUM - 1; `keys` is the width of a
// counter plane.  One round per key present: the first remaining lane's key, a ballot of the lanes on it, popcounts and a shuffle tree
// per sum, and the key's first lane adds with 64-bit atomics.  Integer sums: the totals do not depend on arrival order, nor on the order
// in which a wavefront's keys are visited.
template <int NSUM>
__device__ inline void books_book_wave(int key, bool won, bool lost, const long long (&sums)[NSUM], unsigned long long *__restrict__ counters, int keys) {
    const int lane = threadIdx.x & 63;
    unsigned long long rest = __ballot(key >= 0);
    while (rest) {  // (uniform) none in the usual case
        const int c = __shfl(key, __ffsll(rest) - 1);
        const bool mine = key == c;
        const unsigned long long m = __ballot(mine);
        const unsigned long long mw = __ballot(mine && won), ml = __ballot(mine && lost);
        long long total[NSUM];
#pragma unroll
        for (int k = 0; k < NSUM; k++) total[k] = wave_sum(mine ? sums[k] : 0ll);
        if (lane == __ffsll(m) - 1) {
            const unsigned long long e = (unsigned long long)__popcll(m), nw = (unsigned long long)__popcll(mw), nl = (unsigned long long)__popcll(ml);
            atomicAdd(&counters[kBEpisodes * keys + c], e);
            if (nw) atomicAdd(&counters[kBWins * keys + c], nw);
            if (nl) atomicAdd(&counters[kBLosses * keys + c], nl);
            if (e - nw - nl) atomicAdd(&counters[kBDraws * keys + c], e - nw - nl);
#pragma unroll
            for (int k = 0; k < NSUM; k++) atomicAdd(&counters[(kBReturnSum + k) * keys + c], (unsigned long long)total[k]);
        }
        rest &= ~m;
    }
}

// a fresh draw for env i: a table without a draw (Traits::draw < 0) keeps the ids and the counter
template <class T>
__device__ inline void books_redraw(int32_t *ids, uint32_t *__restrict__ draw_ctr, const uint32_t *__restrict__ w, uint64_t seed, uint64_t gid) {
    const uint32_t ctr = *draw_ctr;
    const int drawn = T::draw(w, seed, gid, ctr);
    if (drawn >= 0) T::put(drawn, ids), *draw_ctr = ctr + 1;
}

// One launch per step with one lane per env.  Episode ends are rare (one step in several hundred per env), so a wavefront without one
// leaves after its loads and stores; one with some books them by the keys actually present (books_book_wave).
// `ids_in` are the ids that PLAYED the step; `ids_out` (it may be `ids_in`) the same, redrawn where `done` is set and `redraw` is.
template <class T>
__global__ __launch_bounds__(kBThreads) void books_step_kernel(int agents, const int32_t *ids_in, const float *__restrict__ reward, int64_t reward_stride,
                                                              const uint8_t *__restrict__ done, int redraw, int32_t *__restrict__ ret,
                                                              int32_t *__restrict__ len, uint32_t *__restrict__ draw_ctr,
                                                              unsigned long long *__restrict__ counters, const uint32_t *__restrict__ w, uint64_t seed,
                                                              int64_t env_id_base, int64_t n, int32_t *ids_out) {
    const int64_t i = (int64_t)blockIdx.x * kBThreads + threadIdx.x;
    int key = -1;  // the key this lane's finished episode goes to; -2: an id outside the pool; -1: no episode ended here
    int r = 0, steps = 0;
    if (i < n) {
        int32_t ids[T::kIds];
#pragma unroll
        for (int k = 0; k < T::kIds; k++) ids[k] = ids_in[T::kIds * i + k];
        r = ret[i] + (int)reward[i * reward_stride];
        steps = len[i] + 1;
        const bool d = done[i] != 0;
        if (d) {
            key = T::key(ids, agents);
            if (redraw) books_redraw<T>(ids, draw_ctr + i, w, seed, (uint64_t)(env_id_base + i));
        }
        ret[i] = d ? 0 : r, len[i] = d ? 0 : steps;
#pragma unroll
        for (int k = 0; k < T::kIds; k++) ids_out[T::kIds * i + k] = ids[k];
    }
    if (!__ballot(key != -1)) return;  // (uniform) the usual case: no episode of this wavefront ended
    const long long sums[2] = {(long long)r, (long long)steps};
    books_book_wave(key, r > 0, r < 0, sums, counters, T::kKeys);
    const unsigned long long stray = __ballot(key == -2);
    if (stray && (int)(threadIdx.x & 63) == __ffsll(stray) - 1) atomicAdd(&counters[kBPlanes * T::kKeys], (unsigned long long)__popcll(stray));
}

// ---- the host object: crl_ledger and crl_arena derive from it
struct Books {
    int device = 0;
    int64_t n = 0, env_id_base = 0;
    uint64_t seed = 0;
    int agents = 0;
    int32_t *ret = nullptr, *len = nullptr;
    uint32_t *draw_ctr = nullptr;
    unsigned long long *counters = nullptr;  // [kBPlanes][kKeys], then `ignored`
    uint32_t *w = nullptr;                   // the weight table
    size_t counter_words = 0, table_words = 0;  // kBPlanes * kKeys; the uint32 words of `w`

    unsigned blocks() const { return (unsigned)((n + kBThreads - 1) / kBThreads); }
};

inline int books_copy(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (dst && src) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return CRL_OK;
}

template <class B>
void books_destroy(B *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->ret) (void)hipFree(b->ret);
    if (b->len) (void)hipFree(b->len);
    if (b->draw_ctr) (void)hipFree(b->draw_ctr);
    if (b->counters) (void)hipFree(b->counters);
    if (b->w) (void)hipFree(b->w);
    delete b;
}

// `what`: the C function's name, for the error text.  `init_table(w, agents)` launches the kernel that writes a fresh pool's table on
// the null stream.  The arguments were checked by the caller.
template <class B, class Init>
int books_create(const char *what, int device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int agents, size_t counter_words,
                 size_t table_words, Init init_table, B **out) {
    HIP_TRY(hipSetDevice(device));
    B *b = new B();
    b->device = device, b->n = num_envs, b->env_id_base = env_id_base, b->seed = seed, b->agents = agents;
    b->counter_words = counter_words, b->table_words = table_words;
    const size_t per_env = (size_t)num_envs * sizeof(int32_t);
    int rc = crl_dev_zalloc(&b->ret, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&b->len, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&b->draw_ctr, per_env, what);
    if (!rc) rc = crl_dev_zalloc(&b->counters, (counter_words + 1) * sizeof(unsigned long long), what);
    if (!rc) rc = crl_dev_zalloc(&b->w, table_words * sizeof(uint32_t), what);
    if (!rc) {
        init_table(b->w, agents);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = crl_hip_fail(e, what);
    }
    if (rc) {
        books_destroy(b);
        return rc;
    }
    *out = b;
    return CRL_OK;
}

inline int books_seed(Books *b, uint64_t seed, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(b->draw_ctr, 0, (size_t)b->n * sizeof(uint32_t), st));
    b->seed = seed;
    return CRL_OK;
}

inline int books_reset(Books *b, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(b->counters, 0, (b->counter_words + 1) * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(b->ret, 0, (size_t)b->n * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(b->len, 0, (size_t)b->n * sizeof(int32_t), st));
    return CRL_OK;
}

// `words`: the table without what a draw keeps behind it (the arena's row sums)
inline int books_get_weights(Books *b, uint32_t *w_out_dev, size_t words, hipStream_t st) {
    return books_copy(w_out_dev, b->w, words * sizeof(uint32_t), st);
}

inline int books_get_counters(Books *b, int64_t *counters_out_dev, int64_t *ignored_out_dev, hipStream_t st) {
    int rc = books_copy(counters_out_dev, b->counters, b->counter_words * sizeof(int64_t), st);
    return rc != CRL_OK ? rc : books_copy(ignored_out_dev, b->counters + b->counter_words, sizeof(int64_t), st);
}

inline int books_set_counters(Books *b, const int64_t *counters_dev, const int64_t *ignored_dev, hipStream_t st) {
    int rc = books_copy(b->counters, counters_dev, b->counter_words * sizeof(int64_t), st);
    return rc != CRL_OK ? rc : books_copy(b->counters + b->counter_words, ignored_dev, sizeof(int64_t), st);
}

inline int books_get_env_state(Books *b, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, hipStream_t st) {
    const size_t bytes = (size_t)b->n * sizeof(int32_t);
    int rc = books_copy(ret_out_dev, b->ret, bytes, st);
    if (rc == CRL_OK) rc = books_copy(len_out_dev, b->len, bytes, st);
    return rc != CRL_OK ? rc : books_copy(draw_ctr_out_dev, b->draw_ctr, bytes, st);
}

inline int books_set_env_state(Books *b, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, hipStream_t st) {
    const size_t bytes = (size_t)b->n * sizeof(int32_t);
    int rc = books_copy(b->ret, ret_dev, bytes, st);
    if (rc == CRL_OK) rc = books_copy(b->len, len_dev, bytes, st);
    return rc != CRL_OK ? rc : books_copy(b->draw_ctr, draw_ctr_dev, bytes, st);
}

// ---- the table of one weight per agent behind crl_ledger_* and crl_car_league_* (pong_ledger.hip).  `who`: the C function's name;
// `w`: the table's kBAgents words on the device; `agents`: the pool's size; the null checks are the caller's.
// crl_*_set_weights: `count` host weights, one per agent of the pool, whose sum lies in [1, 2^32)
int books_set_weights16(const char *who, uint32_t *w, int agents, const uint32_t *w_host, int32_t count, hipStream_t st);
// crl_*_pfsp_weights (include/crl.h "PFSP weights") from `counters_dev`, or from the object's `own` counters where that is null
int books_pfsp16(const char *who, uint32_t *w, int agents, const unsigned long long *own, const int64_t *counters_dev, int32_t mode, int32_t exponent,
                 uint32_t floor, hipStream_t st);

template <class T>
int books_step(Books *b, const int32_t *ids_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev, int redraw, int32_t *ids_out_dev,
               hipStream_t st) {
    hipLaunchKernelGGL(books_step_kernel<T>, dim3(b->blocks()), dim3(kBThreads), 0, st, b->agents, ids_dev, reward_dev, reward_stride, done_dev, redraw,
                       b->ret, b->len, b->draw_ctr, b->counters, b->w, b->seed, b->env_id_base, b->n, ids_out_dev);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

}  // namespace crl

// rollout_core.h -- what the two rollout storages (pong_rollout.hip: planes in separate arrays; car_rollout.hip: one 128-byte line per
// sample) and the learners that read them (pong_ppo.h, car_learner.h) share, each once: the step counters with their refusals, one step
// of the GAE rule, the normalised advantage and the advantages' statistics.  Where a sample's words lie stays the storage's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crl_internal.h"

namespace crl {

enum RolloutState { kFresh = 0, kActive = 1, kFinished = 2 };
// The step counters: crl_rollout and crl_car_rollout derive from it.  The checks are the entry points' refusals (defined in
// pong_rollout.hip): each calls crl_fail itself and returns its code.  `who`: the calling C function's name, crl_<storage>_<call>.
struct RolloutSteps {
    int steps = 0;  // T
    int state = kFresh;
    int recorded = 0, outcomes = 0;  // steps that have their record / their outcome
    bool normalize = false;          // the last finish computed the statistics

    int check_record(const char *who, int64_t t) const;   // t is the next step to record
    int check_outcome(const char *who, int64_t t) const;  // t has its record and not yet its outcome
    int check_finish(const char *who) const;              // every step has its outcome
    int check_finished(const char *who) const;            // a finish has computed what a sample holds
    int check_restore(const char *who, const int32_t *info4) const;  // info4 = state, recorded, outcomes, normalize fits T steps
    void restore(const int32_t *info4) { state = info4[0], recorded = info4[1], outcomes = info4[2], normalize = info4[3] != 0; }
    void info(int32_t *out4) const;  // as restore takes it; the counters read 0 when fresh and T when finished
};

// include/crl.h "GAE rule", one step of the walk t = T-1 .. 0 (acc = 0 and vnext = the value after the last step in front of T-1):
// float32, one rounding per operation; adv and ret are the step's stores
__device__ inline void gae_step(float reward, float v, bool done, float g, float gl, float &acc, float &vnext, float &adv, float &ret) {
#pragma clang fp contract(off)
    const float nd = done ? 0.0f : 1.0f;
    const float delta = (reward + (g * vnext) * nd) - v;
    acc = delta + (gl * nd) * acc;
    adv = acc;
    ret = acc + v;
    vnext = v;
}

// the advantage as a gather hands it out and as a gradient reads it; stats: mean, std when the finish normalised, else null
__device__ inline float adv_out(float adv, const double *stats) {
    return stats ? (adv - (float)stats[0]) / ((float)stats[1] + 1e-5f) : adv;  // float32, true division
}

// ---- the statistics, float64, over a source trait Src that a launch carries by value:
//   static constexpr bool kCounted   samples can be dead: the live ones are counted, L = their count, kept in stats[2]
//   bool live(int64_t i) const       sample i takes part (not counted: true)
//   float adv(int64_t i) const       its advantage
// A statistics buffer is mean, std[, L], then kRedGroups partial sums[, then kRedGroups partial counts].
static constexpr int kRedBlock = 256;  // the fixed shape: at most kRedGroups workgroups of kRedBlock lanes, then one of kRedGroups
static constexpr int kRedGroups = 256;
static_assert(kRedBlock == kRedGroups, "one tree serves both stages");
template <class Src> constexpr int kStatsDoubles = 2 + Src::kCounted + (1 + Src::kCounted) * kRedGroups;

// the fixed tree over the workgroup's values in LDS (and their counts): lane 0's slot holds the sum
template <bool COUNTED> __device__ inline void stats_tree(double *s, double *c) {
    __syncthreads();
    for (int w = kRedBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s[threadIdx.x] += s[threadIdx.x + w];
            if constexpr (COUNTED) c[threadIdx.x] += c[threadIdx.x + w];
        }
        __syncthreads();
    }
}

// The partial sums: workgroup w of `groups` sums (adv - shift)^(1 or 2) over the samples w * 256 + lane, + groups * 256, ... in order
// -- a dead sample contributes 0 --, then the tree.  The first pass of a counted source counts the live samples the same way (an
// integer held in a double: exact).  No atomics: the same samples give the same bits.
template <class Src, bool SQUARE>
__global__ __launch_bounds__(kRedBlock) void rollout_stats_partial_kernel(Src src, int64_t count, const double *__restrict__ stats,
                                                                         double *__restrict__ partials, double *__restrict__ live_partials) {
    __shared__ double s[kRedBlock], c[Src::kCounted ? kRedBlock : 1];
    const double shift = SQUARE ? stats[0] : 0.0;
    double sum = 0.0, cnt = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kRedBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kRedBlock) {
        if (!src.live(i)) continue;
        const double v = (double)src.adv(i) - shift;
        sum += SQUARE ? v * v : v;
        cnt += 1.0;
    }
    s[threadIdx.x] = sum;
    if constexpr (Src::kCounted) c[threadIdx.x] = cnt;
    stats_tree<Src::kCounted>(s, c);
    if (threadIdx.x != 0) return;
    partials[blockIdx.x] = s[0];
    if constexpr (Src::kCounted && !SQUARE) live_partials[blockIdx.x] = c[0];
}

// ... and the one final workgroup.  L = the live count (summed here in the first pass) or `count`; stats[0] = sum / L (0 where L = 0),
// or stats[1] = sqrt(sum / (L - 1)), the unbiased deviation (0 where L < 2, which has none)
template <bool COUNTED, bool SQUARE>
__global__ __launch_bounds__(kRedGroups) void rollout_stats_final_kernel(const double *__restrict__ partials, const double *__restrict__ live_partials,
                                                                        int groups, int64_t count, double *__restrict__ stats) {
    __shared__ double s[kRedGroups], c[COUNTED ? kRedGroups : 1];
    s[threadIdx.x] = (int)threadIdx.x < groups ? partials[threadIdx.x] : 0.0;
    if constexpr (COUNTED) c[threadIdx.x] = (!SQUARE && (int)threadIdx.x < groups) ? live_partials[threadIdx.x] : 0.0;
    stats_tree<COUNTED>(s, c);
    if (threadIdx.x != 0) return;
    double L = (double)count;
    if constexpr (COUNTED) L = SQUARE ? stats[2] : c[0];
    if constexpr (COUNTED && !SQUARE) stats[2] = L;
    if (SQUARE) stats[1] = L > 1.0 ? sqrt(s[0] / (L - 1.0)) : 0.0;
    else stats[0] = L > 0.0 ? s[0] / L : 0.0;
}

// the mean, then the deviation about it, of `count` samples into `stats` (kStatsDoubles<Src> doubles): four launches on `st`
template <class Src> hipError_t rollout_stats_launch(const Src &src, int64_t count, double *stats, hipStream_t st) {
    const int64_t blocks = (count + kRedBlock - 1) / kRedBlock;
    const int groups = (int)(blocks < kRedGroups ? blocks : kRedGroups);
    double *partials = stats + 2 + Src::kCounted, *live = Src::kCounted ? partials + kRedGroups : nullptr;
    hipLaunchKernelGGL((rollout_stats_partial_kernel<Src, false>), dim3(groups), dim3(kRedBlock), 0, st, src, count, stats, partials, live);
    hipLaunchKernelGGL((rollout_stats_final_kernel<Src::kCounted, false>), dim3(1), dim3(kRedGroups), 0, st, partials, live, groups, count, stats);
    hipLaunchKernelGGL((rollout_stats_partial_kernel<Src, true>), dim3(groups), dim3(kRedBlock), 0, st, src, count, stats, partials, live);
    hipLaunchKernelGGL((rollout_stats_final_kernel<Src::kCounted, true>), dim3(1), dim3(kRedGroups), 0, st, partials, live, groups, count, stats);
    return hipGetLastError();
}

static inline unsigned blocks_of(int64_t lanes) { return (unsigned)((lanes + 255) / 256); }  // workgroups of 256 for a lane per item

}  // namespace crl

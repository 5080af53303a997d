// car_learner.h -- what the CarRacing learner's two halves share (include/crl.h "car rollout storage", "car ppo update"): the sample
// line of car_rollout.hip as car_ppo.hip fetches it, and the view of a storage that a gradient launch carries.
//
// ONE SAMPLE = ONE ALIGNED 128-BYTE LINE of 32 words.  The update fetches samples by random index, so everything a gradient lane needs
// of a sample lies in the one line it touches; GAE's strided walk over t costs T * R lines once per rollout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crl_internal.h"
#include "rollout_core.h"  // adv_out: the advantage as crl_car_rollout_gather hands it out

namespace crl {

static constexpr int kCarLineWords = 32;  // 128 bytes
// word offsets inside a line
static constexpr int kCarLineObs = 0;      // [21] the observation
static constexpr int kCarLineU = 21;       // [2] the action as written (unclipped)
static constexpr int kCarLineLogp = 23, kCarLineValue = 24, kCarLineReward = 25, kCarLineReturn = 26, kCarLineAdv = 27;
static constexpr int kCarLineFlags = 28;   // uint32: bit 0 live, bit 1 done
static constexpr uint32_t kCarFlagLive = 1u, kCarFlagDone = 2u;
static_assert(CRL_CAR_OBS_FEATURES == 21 && kCarLineFlags < kCarLineWords, "the line of include/crl.h \"car rollout storage\"");

// a finished storage as a gradient launch sees it
struct CarRolloutView {
    const float *lines;   // [T * R][32]
    const double *stats;  // mean, std of the live advantages (read when the finish normalised), else null
    uint32_t last;        // T * R - 1
    bool finished;
};

CarRolloutView car_rollout_view(const ::crl_car_rollout *r);

}  // namespace crl

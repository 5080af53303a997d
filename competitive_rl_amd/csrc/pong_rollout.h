// pong_rollout.h -- what pong_ppo.hip (the learner's update) reads of a crl_rollout (pong_rollout.hip): the stored planes, the depths
// and the per-sample scalars of a FINISHED rollout, as device pointers.  Read-only: the update rebuilds a sample's stack from the planes
// by the stack rule of include/crl.h itself and never goes through the float32 gather.
#pragma once
#include <stdint.h>

struct crl_rollout;

namespace crl {

struct RolloutView {
    const uint8_t *planes;  // [T + 3][n][kPlanePad]: row t + j is plane j of sample (t, e)
    const uint8_t *depth;   // [T * n]: plane j is live iff 3 - j < depth
    const int32_t *actions;
    const float *logp, *ret, *adv;  // [T * n]
    const double *stats;            // mean, std of the advantages when the finish normalised, else null
    uint32_t n, last;               // last = T * n - 1
    bool finished;
};

RolloutView rollout_view(const crl_rollout *r);

}  // namespace crl

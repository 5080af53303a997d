// pong_ppo.h -- what the two learners (pong_ppo.hip: the LightActorCritic, pong_ppo_full.hip: the full-size ActorCritic) share: the
// crl_ppo object, the per-sample closed forms of include/crl.h "ppo update" and the byte / 255 of the gradient kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crl_internal.h"
#include "pong_rollout.h"

namespace crl {

static constexpr int kStatN = 5;  // policy loss, value loss, entropy, old_logp - logp, clipped

struct PpoHyperDev {
    float clip, vf, ent;
};

struct PpoFull;  // pong_ppo_full.hip: the full-size learner's scratch and accumulators

__device__ inline float div255(float b) {  // b / 255, correctly rounded (Markstein), as the forward kernel forms it
    const float rcp = 1.0f / 255.0f;
    const float qv = b * rcp;
    const float rem = __builtin_fmaf(qv, -255.0f, b);
    return __builtin_fmaf(rem, rcp, qv);
}

// One sample's loss terms from its float64 logits l and value v: dl = d loss_b / d logits and dv = d loss_b / d v, rounded once to
// float32, and the sample's five statistics.
__device__ inline void ppo_sample_terms(const double (&l)[3], const double v, const int act, const double olp, const double ret, const double A,
                                        const PpoHyperDev &h, float (&dl)[3], float &dv, double (&st)[kStatN]) {
    const double m = fmax(fmax(l[0], l[1]), l[2]);
    const double d[3] = {l[0] - m, l[1] - m, l[2] - m};
    const double ex[3] = {exp(d[0]), exp(d[1]), exp(d[2])};
    const double S = (ex[0] + ex[1]) + ex[2];
    const double logS = log(S);
    const double lp[3] = {d[0] - logS, d[1] - logS, d[2] - logS};
    const double p[3] = {ex[0] / S, ex[1] / S, ex[2] / S};
    const double logp = lp[act];
    const double ratio = exp(logp - olp);
    const double lo = 1.0 - (double)h.clip, hi = 1.0 + (double)h.clip;
    const double surr1 = ratio * A, surr2 = fmin(fmax(ratio, lo), hi) * A;
    const bool active = (A >= 0.0 && ratio < hi) || (A < 0.0 && ratio > lo);
    const double glp = active ? -(A * ratio) : 0.0;
    const double H = -((p[0] * lp[0] + p[1] * lp[1]) + p[2] * lp[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) dl[k] = (float)(glp * ((k == act ? 1.0 : 0.0) - p[k]) + (double)h.ent * (p[k] * (lp[k] + H)));
    const double dif = v - ret;
    dv = (float)((double)h.vf * dif);
    st[0] = -fmin(surr1, surr2), st[1] = 0.5 * (dif * dif), st[2] = H;
    st[3] = olp - logp, st[4] = (ratio < lo || ratio > hi) ? 1.0 : 0.0;
}

// the full-size learner behind the common entry points of pong_ppo.hip (p->full is set)
void ppo_full_destroy(PpoFull *f);
int64_t ppo_full_scratch_rows(const PpoFull *f);  // samples per chunk of a minibatch: part of the summation shape (crl_ppo_get_state)
int ppo_full_grad(::crl_ppo *p, const RolloutView &view, const int64_t *idx_dev, int64_t count, const PpoHyperDev &h, hipStream_t st);

}  // namespace crl

struct crl_ppo {
    int device = 0;
    int blob_floats = 0;  // the master blob, both moments and the gradient: 8 488 floats (light) or 1 001 784 (full size)
    float *raw = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr;
    double *red = nullptr;  // [0]: the gradient's sum of squares, [1 .. 5]: the statistics' means
    float *partials = nullptr;                        // light: [W][blob]
    double *stat_part = nullptr, *sq_part = nullptr;  // light
    crl::PpoFull *full = nullptr;                     // crl_ppo_create_full
    int64_t steps = 0;  // optimiser steps taken (the t of the bias corrections)
    bool have_grad = false;
};

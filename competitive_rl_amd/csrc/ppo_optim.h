// ppo_optim.h -- what every learner's optimiser shares and what does not know the network (pong_ppo.hip, pong_ppo_full.hip, car_ppo.hip):
// the four blobs of a learner (master weights, Adam's two moments, the gradient) with their host helpers, the check of the
// hyper-parameters, and the optimiser step of include/crl.h "ppo update" as one lane's statements.  A learner's step kernel is a thin
// caller of adam_lane: it knows where the gradient's sum of squares lies and what follows the new parameter.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crl_internal.h"

namespace crl {

// the blobs as a step kernel's lane sees them
struct AdamBlobs {
    float *raw, *m, *v;
    const float *grad;
};

// crl_ppo and crl_car_ppo derive from it
struct PpoBlobs {
    int device = 0;
    int blob_floats = 0;  // the master blob, both moments and the gradient: 8 488 floats (light), 1 001 784 (full size) or 2 508 (car)
    float *raw = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr;
    int64_t steps = 0;  // optimiser steps taken (the t of the bias corrections)
    bool have_grad = false;

    AdamBlobs adam() const { return AdamBlobs{raw, m, v, grad}; }
};

struct AdamArgs {
    float max_norm, b1, b2, omb1, omb2, step_size, bc2_sqrt, eps;
};

// the bias corrections of step t (1-based) in float64, rounded once: 1 - b1, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t)
inline AdamArgs adam_args(const crl_ppo_hyper *hyper, int64_t t) {
    const double b1 = (double)hyper->beta1, b2 = (double)hyper->beta2;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    return AdamArgs{hyper->max_grad_norm, hyper->beta1, hyper->beta2, (float)(1.0 - b1), (float)(1.0 - b2), (float)((double)hyper->lr / bc1),
                    (float)sqrt(bc2), hyper->eps};
}

// include/crl.h "ppo update", optimiser step, for float i of the blobs: float32, one rounding per operation (no contraction; sqrtf and /
// correctly rounded).  `sq`: the gradient's sum of squares.  Stores both moments and returns the new parameter.
__device__ inline float adam_lane(const AdamArgs &h, const AdamBlobs &b, int i, double sq) {
#pragma clang fp contract(off)
    const float norm = (float)sqrt(sq);
    const float coef = fminf(1.0f, h.max_norm / (norm + 1e-6f));
    const float g = b.grad[i] * coef;
    const float m = h.b1 * b.m[i] + h.omb1 * g;
    const float v = h.b2 * b.v[i] + h.omb2 * (g * g);
    b.m[i] = m, b.v[i] = v;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    return b.raw[i] - h.step_size * (m / denom);
}

// ---- the host side (pong_ppo.hip).  `who`: the C function's name, for the error text.
int ppo_hyper_check(const char *who, const crl_ppo_hyper *h);
// raw, m, v, grad of blob_floats floats, zeroed
int ppo_alloc_blobs(PpoBlobs *p, int blob_floats, const char *who);
void ppo_free_blobs(PpoBlobs *p);
// a packed host blob becomes the master weights; both moments and the step count go to zero (synchronises)
int ppo_upload(PpoBlobs *p, const float *blob);
// the master blob on the host (synchronises)
int ppo_download(PpoBlobs *p, float *blob);
// the bodies of crl_*_ppo_get_grad / get_state / set_state behind the caller's argument checks
int ppo_read_grad(PpoBlobs *p, const float **grad_dev, float *grad_out_host);
int ppo_read_state(PpoBlobs *p, float *blob_out_host, float *m_out_host, float *v_out_host, int64_t *steps_out, hipStream_t st);
int ppo_write_state(PpoBlobs *p, const float *blob_host, const float *m_host, const float *v_host, int64_t steps, hipStream_t st);

}  // namespace crl

// pong_sample.h -- the action epilogue of a served agent (action_epilogue: argmax or draw, and the stores) and include/crl.h
// "sampled actions" for one that does not play greedy: one Philox call by the lane that writes the action.  Shared by the
// LightActorCritic kernels (pong_policy.hip), the full-size actor (pong_policy_full.hip) and RULE_BASED's explore branch
// (pong_league.hip).
#pragma once
#include <math.h>

#include "crl_internal.h"
#include "pong_device.h"

namespace crl {

// What a launch with sampling carries (kernel arguments: nothing of it lives in device memory).
struct SampleArgs {
    uint64_t seed;    // the key
    int64_t id_base;  // global id of env 0 of the launch's arrays
    uint32_t n;       // act calls since create / seed: the counter RANDOM's action uses
    uint32_t eps_q;   // min(floor(epsilon * 2^32), 0xFFFFFFFF)
    float inv_t;      // float32 1 / temperature; 0 = greedy where the draw does not explore
};

// host: the launch parameters of a (temperature, epsilon) pair, or CRL_EINVAL -- looked at before any GPU call
inline int sample_args_from(float temperature, float epsilon, const char *what, SampleArgs *out) {
    if (!(temperature >= 0.f) || !isfinite(temperature)) return crl_fail(CRL_EINVAL, "%s: temperature must be finite and >= 0, not %g", what, (double)temperature);
    if (!(epsilon >= 0.f && epsilon <= 1.f)) return crl_fail(CRL_EINVAL, "%s: epsilon must lie in [0, 1], not %g", what, (double)epsilon);
    const float inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
    if (!isfinite(inv_t)) return crl_fail(CRL_EINVAL, "%s: temperature %g is too small, 1 / temperature is no float32", what, (double)temperature);
    const double q = floor((double)epsilon * 4294967296.0);
    out->eps_q = q >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)q;
    out->inv_t = inv_t;
    return CRL_OK;
}

// 1. explore: the explore action, or -1 (x0 is then the word step 3 uses)
__device__ inline int sample_explore(uint64_t seed, uint64_t gid, uint32_t n, uint32_t eps_q, uint32_t &x0) {
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), n, CRL_LEAGUE_DOMAIN_SAMPLE};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    x0 = c[0];
    return c[1] < eps_q ? (int)(((uint64_t)c[2] * 3u) >> 32) : -1;
}

// `greedy`: the first-index argmax of (l0, l1, l2), which the caller has anyway
__device__ inline int sample_action(const SampleArgs &S, int64_t env, float l0, float l1, float l2, int greedy) {
    uint32_t x0;
    const int explored = sample_explore(S.seed, (uint64_t)(S.id_base + env), S.n, S.eps_q, x0);
    if (explored >= 0) return explored;
    if (S.inv_t == 0.f) return greedy;
    const float z0 = l0 * S.inv_t, z1 = l1 * S.inv_t, z2 = l2 * S.inv_t;
    const float m = fmaxf(fmaxf(z0, z1), z2);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m), e2 = expf(z2 - m);
    const float e01 = e0 + e1, sum = e01 + e2;
    const float rs = ((float)(x0 >> 8) * 0x1p-24f) * sum;
    return rs < e0 ? 0 : rs < e01 ? 1 : 2;
}

// host: does an agent with these parameters need the SAMPLE kernels?  (0, 0) -- every agent, until it is set -- keeps the greedy ones
inline bool sample_active(const SampleArgs &S) { return S.inv_t != 0.f || S.eps_q != 0; }

// What the lane that holds an env's three logits does with them: the first-index argmax (torch.argmax; a NaN logit is no supported
// input and is not guarded), SAMPLE: the draw instead, then the action and, where asked for, the logits.  SAMPLE is a template
// parameter, not a branch on a kernel argument: the greedy kernels are the code they were, whatever the compiler makes of the draw.
template <bool SAMPLE>
__device__ __forceinline__ void action_epilogue(const SampleArgs &S, int64_t env, float a0, float a1, float a2, int32_t *__restrict__ actions,
                                                int64_t action_stride, float *__restrict__ logits) {
    int best = 0;
    float bv = a0;
    if (a1 > bv) best = 1, bv = a1;
    if (a2 > bv) best = 2;
    if constexpr (SAMPLE) best = sample_action(S, env, a0, a1, a2, best);
    actions[env * action_stride] = best;
    if (logits) {
        float *lo = logits + env * 3;
        lo[0] = a0, lo[1] = a1, lo[2] = a2;
    }
}

}  // namespace crl

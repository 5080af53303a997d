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

// What a rollout launch (crl_policy_act_rollout with values or log-probs) carries beside the actor: the critic row and where the two
// extra heads go.  The other launches pass it zeroed and never read it.
struct HeadArgs {
    const float *wc, *bc;  // critic_linear: [1600] (light) / [256] (full-size) and [1], device
    float *values;         // optional float32 [N]: critic_linear(features)
    float *logp;           // optional float32 [N]: include/crl.h "rollout heads"
};

// include/crl.h "rollout heads": step 3 of "sampled actions" with its terms kept -- d_a = z_a - m, e_a = expf(d_a), S = (e0 + e1) + e2
// are formed ONCE and serve the draw and the log-probability both.  inv_t is 1 where the style has no temperature.
struct SoftmaxTerms {
    float d0, d1, d2, e0, e01, sum;
};
__device__ inline SoftmaxTerms softmax_terms(float l0, float l1, float l2, float inv_t) {
    const float z0 = l0 * inv_t, z1 = l1 * inv_t, z2 = l2 * inv_t;
    const float m = fmaxf(fmaxf(z0, z1), z2);
    SoftmaxTerms t;
    t.d0 = z0 - m, t.d1 = z1 - m, t.d2 = z2 - m;
    const float e0 = expf(t.d0), e1 = expf(t.d1), e2 = expf(t.d2);
    t.e0 = e0, t.e01 = e0 + e1, t.sum = t.e01 + e2;
    return t;
}

// host: does an agent with these parameters need the SAMPLE kernels?  (0, 0) -- every agent, until it is set -- keeps the greedy ones
inline bool sample_active(const SampleArgs &S) { return S.inv_t != 0.f || S.eps_q != 0; }

// What the lane that holds an env's three logits does with them: the first-index argmax (torch.argmax; a NaN logit is no supported
// input and is not guarded), SAMPLE: the draw instead, then the action and, where asked for, the logits.  SAMPLE is a template
// parameter, not a branch on a kernel argument: the greedy kernels are the code they were, whatever the compiler makes of the draw.
// HEADS (the rollout launches): the value `v` and the log-probability of the action written, whichever branch chose it, go out as
// well (H.values / H.logp, each optional); the softmax terms are formed once for the draw and the log-probability.  A template
// parameter for the same reason: action_epilogue<SAMPLE> is the code it was.
template <bool SAMPLE, bool HEADS = false>
__device__ __forceinline__ void action_epilogue(const SampleArgs &S, int64_t env, float a0, float a1, float a2, int32_t *__restrict__ actions,
                                                int64_t action_stride, float *__restrict__ logits, float v = 0.f, const HeadArgs *H = nullptr) {
    int best = 0;
    float bv = a0;
    if (a1 > bv) best = 1, bv = a1;
    if (a2 > bv) best = 2;
    if constexpr (HEADS) {
        const bool tempered = SAMPLE && S.inv_t != 0.f;
        const SoftmaxTerms t = softmax_terms(a0, a1, a2, tempered ? S.inv_t : 1.0f);
        if constexpr (SAMPLE) {
            uint32_t x0;
            const int explored = sample_explore(S.seed, (uint64_t)(S.id_base + env), S.n, S.eps_q, x0);
            if (explored >= 0) best = explored;
            else if (tempered) {
                const float rs = ((float)(x0 >> 8) * 0x1p-24f) * t.sum;
                best = rs < t.e0 ? 0 : rs < t.e01 ? 1 : 2;
            }
        }
        if (H->values) H->values[env] = v;
        if (H->logp) H->logp[env] = (best == 0 ? t.d0 : best == 1 ? t.d1 : t.d2) - logf(t.sum);
    } else if constexpr (SAMPLE) best = sample_action(S, env, a0, a1, a2, best);
    actions[env * action_stride] = best;
    if (logits) {
        float *lo = logits + env * 3;
        lo[0] = a0, lo[1] = a1, lo[2] = a2;
    }
}

}  // namespace crl

// pong_ppo.h -- what the two learners (pong_ppo.hip: the LightActorCritic, pong_ppo_full.hip: the full-size ActorCritic) share: the
// crl_ppo object and its host helpers (the four blobs), the reduce kernel, the sample fetch (which sample is row i of idx, its
// scalars, its planes by the stack rule), the per-sample closed forms of include/crl.h "ppo update" with or without a teacher, and the
// byte / 255 of the gradient kernels.  The blobs' helpers, the hyper-parameter check and the optimiser step are ppo_optim.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crl_internal.h"
#include "pong_ring.h"
#include "pong_rollout.h"
#include "rollout_core.h"
#include "ppo_optim.h"

namespace crl {

static constexpr int kStatN = 5;  // policy loss, value loss, entropy, old_logp - logp, clipped
// ---- include/crl.h "ppo update, teacher targets"
static constexpr int kStatT = 4;                // ce, kl to the teacher, agreement, labelled
static constexpr int kStatAll = kStatN + kStatT;  // what a teacher gradient's statistics carry

struct PpoHyperDev {
    float clip, vf, ent;
};

struct PpoTeacherDev {
    const float *logits;    // [T * N][3] or null
    const int32_t *labels;  // [T * N] or null: exactly one of the two
    const float *vtarget;   // [T * N] or null = the stored returns
    float tau, coef;
    int32_t policy_term;
};

// what a teacher instantiation of a heads kernel receives where the plain one receives PpoHyperDev (built as PpoHyperTeacher{h, t})
struct PpoHyperTeacher : PpoHyperDev {
    PpoTeacherDev t;
};

struct PpoFull;  // pong_ppo_full.hip: the full-size learner's scratch and accumulators

__device__ inline float div255(float b) {  // b / 255, correctly rounded (Markstein), as the forward kernel forms it
    const float rcp = 1.0f / 255.0f;
    const float qv = b * rcp;
    const float rem = __builtin_fmaf(qv, -255.0f, b);
    return __builtin_fmaf(rem, rcp, qv);
}

// ---- the sample fetch.  Everything of a sample is read at its FLAT index t * n + e, never at its place in the batch.
// the flat index of row `row` of idx (a bad index only reads inside the arrays, as in the gather)
__device__ inline uint32_t sample_of(const RolloutView &r, const int64_t *idx, int64_t row) {
    const uint32_t raw = (uint32_t)idx[row];
    return raw < r.last ? raw : r.last;
}

// the stack rule: plane j of the sample's stack is row t + j of the planes (live iff CRL_POLICY_STACK - 1 - j < depth; a masked plane
// reads as zeros)
struct SampleAt {
    uint32_t t, e;  // flat = t * n + e: formed once per sample (a 32-bit divide)
};
__device__ inline SampleAt sample_at(const RolloutView &r, uint32_t flat) {
    const uint32_t t = flat / r.n;
    return SampleAt{t, flat - t * r.n};
}
// ... chunk c of its kPlaneChunks 16-byte chunks
__device__ inline const uint4 *plane_of(const RolloutView &r, SampleAt at, int j, int c = 0) {
    return reinterpret_cast<const uint4 *>(r.planes) + (((int64_t)(at.t + j) * r.n + at.e) * kPlaneChunks + c);
}

// One sample's teacher row as the kernels stage it: the three logits (or nothing) and the label (-1: none; logits: not read)
struct TeacherRow {
    float l[3] = {0.f, 0.f, 0.f};
    int32_t label = -1;
};

// One sample's scalars; as constructed, what a slot without a sample holds
struct PpoSample {
    int act = 0;                                // clamped to 0 .. 2
    float olp = 0.f, target = 0.f, adv = 0.f;  // old log-prob; value target (the stored return or the teacher's); advantage as crl_rollout_gather hands it out
    TeacherRow tr;
};

// t: null = no teacher (the stored return is the value target, the teacher row stays empty)
__device__ inline PpoSample sample_scalars(const RolloutView &r, uint32_t flat, const PpoTeacherDev *t) {
    PpoSample s;
    const int32_t ai = r.actions[flat];
    s.act = ai < 0 ? 0 : ai > 2 ? 2 : ai;
    s.olp = r.logp[flat], s.target = r.ret[flat], s.adv = r.adv[flat];  // (all loads in flight before the first is waited for)
    s.adv = adv_out(s.adv, r.stats);
    if (t) {
        if (t->logits) s.tr.l[0] = t->logits[3 * (int64_t)flat], s.tr.l[1] = t->logits[3 * (int64_t)flat + 1], s.tr.l[2] = t->logits[3 * (int64_t)flat + 2];
        else s.tr.label = t->labels[flat];
        if (t->vtarget) s.target = t->vtarget[flat];
    }
    return s;
}

// One sample's loss terms from its float64 logits l and value v: dl = d loss_b / d logits and dv = d loss_b / d v, rounded once to
// float32, and the sample's five statistics.  `ret` is the value target the caller chose.
// TEACHER: with a teacher term from the teacher *t (plain: not read) and the sample's teacher row tr.  dl_k = (the plain expression,
// the policy part at 0 when policy_term is 0) + coef (p_k - q_k), the teacher term added last; st: the five statistics as always, then
// ce, kl, agree, labelled.
template <bool TEACHER>
__device__ inline void ppo_sample_terms(const double (&l)[3], const double v, const int act, const double olp, const double ret, const double A,
                                        const PpoHyperDev &h, [[maybe_unused]] const PpoTeacherDev *t, [[maybe_unused]] const TeacherRow &tr,
                                        float (&dl)[3], float &dv, double (&st)[TEACHER ? kStatAll : kStatN]) {
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
    bool policy = active;
    if constexpr (TEACHER) policy = active && t->policy_term;
    const double glp = policy ? -(A * ratio) : 0.0;
    const double H = -((p[0] * lp[0] + p[1] * lp[1]) + p[2] * lp[2]);
    // the target distribution (no teacher: no sample is labelled, and the teacher term below is not there)
    double q[3] = {0.0, 0.0, 0.0}, ce = 0.0, Hq = 0.0, coef = 0.0;
    bool labelled = false;
    int qtop = 0;
    if constexpr (TEACHER) {
        double qlq[3] = {0.0, 0.0, 0.0};  // q_k log q_k (a term with q_k = 0 counts as 0)
        if (t->logits) {
            const double tau = (double)t->tau;
            const double u[3] = {(double)tr.l[0] / tau, (double)tr.l[1] / tau, (double)tr.l[2] / tau};
            const double mu = fmax(fmax(u[0], u[1]), u[2]);
            const double eu[3] = {exp(u[0] - mu), exp(u[1] - mu), exp(u[2] - mu)};
            const double Su = (eu[0] + eu[1]) + eu[2];
            const double logSu = log(Su);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                q[k] = eu[k] / Su;
                qlq[k] = q[k] > 0.0 ? q[k] * ((u[k] - mu) - logSu) : 0.0;
            }
            qtop = u[1] > u[0] ? 1 : 0;
            if (u[2] > u[qtop]) qtop = 2;
            labelled = true;
        } else {
            labelled = (uint32_t)tr.label < 3u;
            if (labelled) q[tr.label] = 1.0, qtop = tr.label;
        }
        if (labelled) {
            const double c0 = q[0] > 0.0 ? q[0] * lp[0] : 0.0, c1 = q[1] > 0.0 ? q[1] * lp[1] : 0.0, c2 = q[2] > 0.0 ? q[2] * lp[2] : 0.0;
            ce = -((c0 + c1) + c2);
            Hq = -((qlq[0] + qlq[1]) + qlq[2]);
        }
        coef = (double)t->coef;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double base = glp * ((k == act ? 1.0 : 0.0) - p[k]) + (double)h.ent * (p[k] * (lp[k] + H));
        dl[k] = (float)(labelled ? base + coef * (p[k] - q[k]) : base);
    }
    const double dif = v - ret;
    dv = (float)((double)h.vf * dif);
    st[0] = -fmin(surr1, surr2), st[1] = 0.5 * (dif * dif), st[2] = H;
    st[3] = olp - logp, st[4] = (ratio < lo || ratio > hi) ? 1.0 : 0.0;
    if constexpr (TEACHER) {
        int ptop = l[1] > l[0] ? 1 : 0;
        if (l[2] > l[ptop]) ptop = 2;
        st[5] = ce, st[6] = ce - Hq, st[7] = (labelled && ptop == qtop) ? 1.0 : 0.0, st[8] = labelled ? 1.0 : 0.0;
    }
}

// Reduce, either learner's: a lane per element of the BLOB floats adds the `groups` partial blobs [groups][PART] in workgroup order
// (float32) where the partials hold the element (i < PART), else takes the accumulated sum gacc[i] (PART == BLOB: not read), and divides
// by B; the workgroup's 256 squares go through a binary tree in float64 into sq_part[block].
template <int PART, int BLOB>
__global__ __launch_bounds__(256) void ppo_reduce_kernel(const float *__restrict__ partials, int groups, const float *__restrict__ gacc, float count_f,
                                                        float *__restrict__ grad, double *__restrict__ sq_part) {
    __shared__ double s[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float g = 0.f;
    if (i < BLOB) {
        float sum;
        if (i < PART) {
            sum = partials[i];
            for (int w = 1; w < groups; w++) sum += partials[(int64_t)w * PART + i];
        } else {
            sum = gacc[i];
        }
        g = sum / count_f;
        grad[i] = g;
    }
    s[threadIdx.x] = (double)g * (double)g;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq_part[blockIdx.x] = s[0];
}

// the full-size learner behind the common entry points of pong_ppo.hip (p->full is set)
void ppo_full_destroy(PpoFull *f);
int64_t ppo_full_scratch_rows(const PpoFull *f);  // samples per chunk of a minibatch: part of the summation shape (crl_ppo_get_state)
// t: null = the plain gradient (the kernels crl_ppo_grad has always launched), else the teacher instantiations
int ppo_full_grad(::crl_ppo *p, const RolloutView &view, const int64_t *idx_dev, int64_t count, const PpoHyperDev &h, const PpoTeacherDev *t,
                  hipStream_t st);

// either learner's four blobs (ppo_alloc_blobs) and red, zeroed (pong_ppo.hip)
int ppo_alloc(::crl_ppo *p, int blob_floats, const char *who);

}  // namespace crl

struct crl_ppo : crl::PpoBlobs {
    double *red = nullptr;  // [0]: the gradient's sum of squares, [1 .. 5]: the statistics' means, [6 .. 9]: a teacher gradient's four
    float *partials = nullptr;                        // light: [W][blob]
    double *stat_part = nullptr, *sq_part = nullptr;  // light (stat_part: [W][5], a teacher gradient's [W][9])
    crl::PpoFull *full = nullptr;                     // crl_ppo_create_full
    bool teacher_grad = false;  // the last gradient was crl_ppo_grad_teacher's: red[6 .. 9] are its statistics
};

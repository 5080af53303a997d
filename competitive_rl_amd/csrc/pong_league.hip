// pong_league.hip -- per-env opponents for cPongTournament-v0: which agent plays the right-hand bat is an int32 per env ON THE
// DEVICE, the draws of it and of RANDOM's actions are counter-based, and no opponent action touches the host.
//
// Stands in for what a population of the reference's workers does together: every worker's TournamentEnvWrapper draws its own
// opponent (competitive_pong_env.py:27-33 reset_opponent -> random.choice(agent_names)), RANDOM plays np.random.randint(3)
// (builtin_policies.py:51-58), RULE_BASED the cheat code (:44-48), WEAK / MEDIUM a LightActorCritic on the last four frames
// (:61-91, utils/policy_serving.py:46-66).  Here one batch holds the whole population.
//
// A step is: one fill launch (one lane per env: RANDOM's Philox action, 999 for RULE_BASED -- or its explore draw, include/crl.h
// "sampled actions" --, and the frame push of every env that no network visits) and one list launch of pong_policy_mfma_kernel per CNN agent of the pool (weights differ per launch; an agent
// without envs costs an empty persistent launch).  The lists come from the partition kernel, which runs when the assignment
// changed.  ONE ring of the last four opponent-view frames per env serves every CNN agent and is pushed every step whichever agent
// is assigned (one `head` for all envs), so an env that changes hands is judged on the frames it really showed.  Exactly one
// writer per env and step for the ring slot and for the action: the fill kernel for envs of RANDOM / RULE_BASED, the env's own
// agent's list launch otherwise.
//
// Full-size agents (CRL_POOL_KIND_FULL, crl_pool_add_full): the ActorCritic of pong_policy_full.hip on the agent's list, three
// launches per pass (policy_full_act_list).  Each has its own weight blob and list; the activation scratch (act2, feat) is ONE per
// league, shared by all of them -- their launches are ordered on the stream -- and allocated by the first add.
#include <string.h>

#include <vector>

#include "crl_internal.h"
#include "pong_device.h"
#include "pong_league.h"
#include "pong_policy_full.h"
#include "pong_ring.h"
#include "pong_sample.h"

namespace crl {

static constexpr int kLThreads = 256;
static constexpr int kMaxAgents = CRL_LEAGUE_MAX_AGENTS;

struct LeagueExplore {
    uint32_t eps_q[kMaxAgents];  // RULE_BASED agents: the explore threshold of "sampled actions" (0: always the cheat code); 0 for every other kind
};

struct LeagueLists {
    int32_t *list[kMaxAgents];  // CNN agents (light and full-size): env indices of the agent (order free); nullptr for RANDOM / RULE_BASED
};

// Re-draws the opponent of every env (redraw_all) or of the envs whose flag in `done` is set, then rebuilds the per-agent counts and
// the CNN agents' lists: ballot + popcount + one atomic per wavefront and agent (car_step_kernel's coupled list does the same).
__global__ __launch_bounds__(kLThreads) void league_partition_kernel(LeagueLists T, int agents, int32_t *__restrict__ assign,
                                                                    uint32_t *__restrict__ draw_ctr, const uint8_t *__restrict__ done, int redraw_all,
                                                                    uint64_t seed, int64_t env_id_base, int64_t n, unsigned *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * kLThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int a = -1;
    if (i < n) {
        a = assign[i];
        if (redraw_all || (done && done[i])) {
            const uint32_t ctr = draw_ctr[i];
            a = (int)league_draw(seed, (uint64_t)(env_id_base + i), ctr, CRL_LEAGUE_DOMAIN_OPPONENT, (uint32_t)agents);
            draw_ctr[i] = ctr + 1, assign[i] = a;
        }
    }
    for (int k = 0; k < agents; k++) {
        const unsigned long long m = __ballot(a == k);
        if (!m) continue;  // (uniform)
        const int leader = __ffsll(m) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&counts[k], (unsigned)__popcll(m));
        base = __shfl(base, leader);
        if (a == k && T.list[k]) T.list[k][base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
    }
}

// One lane per env.  RANDOM: action = league_draw(.., step, ACTION domain, 3); RULE_BASED (and an id outside the pool): 999, resolved by
// the step kernel -- unless the agent explores (E.eps_q) and this step's sample draw says so.  Then the wavefront pushes the newest frame of each of its envs that no list launch visits into ring plane `head`
// (441 dwords per env, 64 lanes side by side; frames are 4-byte aligned like crl_policy_act's).
__global__ __launch_bounds__(kLThreads) void league_fill_kernel(const int32_t *__restrict__ kinds, int agents, const int32_t *__restrict__ assign,
                                                               uint8_t *__restrict__ ring, int head, const uint8_t *__restrict__ frame, int64_t frame_stride,
                                                               int32_t *__restrict__ actions, int64_t action_stride, uint64_t seed, int64_t env_id_base,
                                                               uint32_t step, int64_t n, LeagueExplore E) {
    const int64_t i = (int64_t)blockIdx.x * kLThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool mine = false;
    if (i < n) {
        const int a = assign[i];
        const int kind = (a >= 0 && a < agents) ? kinds[a] : CRL_LEAGUE_RULE_BASED;
        mine = kind < CRL_LEAGUE_LIGHT;  // CRL_LEAGUE_LIGHT and CRL_POOL_KIND_FULL: a list launch visits the env (action and frame push)
        if (kind == CRL_LEAGUE_RANDOM) actions[i * action_stride] = (int32_t)league_draw(seed, (uint64_t)(env_id_base + i), step, CRL_LEAGUE_DOMAIN_ACTION, 3u);
        else if (mine) {
            int act = CRL_PONG_CHEAT;
            const uint32_t eps_q = (a >= 0 && a < agents) ? E.eps_q[a] : 0u;
            if (eps_q) {
                uint32_t x0;
                const int explored = sample_explore(seed, (uint64_t)(env_id_base + i), step, eps_q, x0);
                if (explored >= 0) act = explored;
            }
            actions[i * action_stride] = act;
        }
    }
    unsigned long long m = __ballot(mine);
    const int64_t w0 = i - lane;
    while (m) {  // (uniform)
        const int b = __ffsll(m) - 1;
        m &= m - 1;
        const int64_t e = w0 + b;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(frame + e * frame_stride);
        uint32_t *dst = reinterpret_cast<uint32_t *>(ring + e * (int64_t)kRingBytes + head * kPlanePad);
#pragma unroll
        for (int q = 0; q < 7; q++) {
            const int d = q * 64 + lane;
            if (d < kPlaneWords) dst[d] = src[d];
        }
    }
}

__global__ void league_fill_assignment_kernel(int32_t *__restrict__ assign, int32_t value, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) assign[i] = value;
}

}  // namespace crl

using namespace crl;

struct crl_league {
    int device = 0;
    int64_t n = 0, n_pad = 0, env_id_base = 0;
    uint64_t seed = 0;
    int cus = 256;
    int head = 0;        // ring plane holding the OLDEST frame (the next one to be replaced), one for all envs
    uint32_t step = 0;   // crl_league_act calls since create / seed: the counter of RANDOM's action draws
    int agents = 0;
    int kind[kMaxAgents] = {};
    float *raw[kMaxAgents] = {};  // CNN agents: the checkpoint tensors (pong_league.h kLightRawFloats; full-size: policy_full_pack's blob)
    int64_t scratch_rows = 0;     // full-size agents: rows of the shared scratch, fixed by the first crl_pool_add_full (0: none yet)
    float *act2 = nullptr, *feat = nullptr;  // ... [scratch_rows][3872] and [scratch_rows][256]
    float temperature[kMaxAgents] = {}, epsilon[kMaxAgents] = {};  // crl_sampling_set_agent, as given
    SampleArgs sample[kMaxAgents] = {};                            // ... and as the launches take it (inv_t, eps_q)
    LeagueLists T{};
    uint8_t *ring = nullptr;
    int32_t *assign = nullptr;
    uint32_t *draw_ctr = nullptr;
    unsigned *ctrl = nullptr;  // [0, 16): tickets of the list launches, [16, 32): counts, [32, 48): kinds (int32)
    WeightStage stage{};       // crl_pool_load_light / _load_full: the pinned host copy of the blob on its way (pong_league.h)
};

static unsigned *league_counts(crl_league *l) { return l->ctrl + kMaxAgents; }
static int32_t *league_kinds(crl_league *l) { return reinterpret_cast<int32_t *>(l->ctrl + 2 * kMaxAgents); }

static int league_partition(crl_league *l, const uint8_t *done_dev, int redraw_all, hipStream_t st) {
    if (l->agents <= 0) return crl_fail(CRL_ESTATE, "crl_league: the pool is empty (crl_league_add_builtin / _add_light first)");
    HIP_TRY(hipMemsetAsync(league_counts(l), 0, kMaxAgents * sizeof(unsigned), st));
    hipLaunchKernelGGL(league_partition_kernel, dim3((unsigned)((l->n + kLThreads - 1) / kLThreads)), dim3(kLThreads), 0, st, l->T, l->agents, l->assign,
                       l->draw_ctr, done_dev, redraw_all, l->seed, l->env_id_base, l->n, league_counts(l));
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

static int league_add(crl_league *l, int kind, const float *raw_host, int64_t scratch_rows = 0) {
    if (l->agents >= kMaxAgents) return crl_fail(CRL_EINVAL, "crl_league: at most %d agents in a pool", kMaxAgents);
    HIP_TRY(hipSetDevice(l->device));
    const int a = l->agents;
    if (kind == CRL_POOL_KIND_FULL && !l->scratch_rows) {  // the first full-size agent: the league's one scratch
        if (int rc = crl_dev_zalloc(&l->act2, (size_t)scratch_rows * policy_full_act2_floats() * sizeof(float), "crl_pool_add_full")) return rc;
        if (int rc = crl_dev_zalloc(&l->feat, (size_t)scratch_rows * policy_full_feat_floats() * sizeof(float), "crl_pool_add_full")) {
            (void)hipFree(l->act2), l->act2 = nullptr;
            return rc;
        }
        l->scratch_rows = scratch_rows;
    }
    if (kind == CRL_POOL_KIND_FULL || kind == CRL_LEAGUE_LIGHT) {  // the CNN agents: the weights and the env list
        const size_t bytes = (kind == CRL_LEAGUE_LIGHT ? (size_t)kLightRawFloats : (size_t)policy_full_blob_floats()) * sizeof(float);
        if (!l->raw[a]) HIP_TRY(hipMalloc(&l->raw[a], bytes));  // (a slot whose add failed half way keeps what it got: destroy frees it)
        HIP_TRY(hipMemcpy(l->raw[a], raw_host, bytes, hipMemcpyHostToDevice));
        if (!l->T.list[a])  // (entries past the count are read, never used)
            if (int rc = crl_dev_zalloc(&l->T.list[a], (size_t)(l->n_pad + 8) * sizeof(int32_t), "crl_league: an agent's env list")) return rc;
        if (kind == CRL_LEAGUE_LIGHT) HIP_TRY(policy_light_prepare());
    }
    l->kind[a] = kind;
    const int32_t k32 = kind;
    HIP_TRY(hipMemcpy(league_kinds(l) + a, &k32, sizeof(k32), hipMemcpyHostToDevice));
    l->agents = a + 1;
    // the assignment in force (all zeros after create) gets its counts and lists for the grown pool
    HIP_TRY(hipDeviceSynchronize());
    int rc = league_partition(l, nullptr, 0, nullptr);
    if (rc != CRL_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return CRL_OK;
}

extern "C" {

int crl_league_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, crl_league **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || num_envs > 0x7fffffff || env_id_base < 0) return crl_fail(CRL_EINVAL, "crl_league_create: bad arguments");
    HIP_TRY(hipSetDevice(device));
    crl_league *l = new crl_league();
    l->device = device, l->n = num_envs, l->n_pad = (num_envs + 7) / 8 * 8, l->env_id_base = env_id_base, l->seed = seed;
    if (hipDeviceGetAttribute(&l->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || l->cus <= 0) l->cus = 256;
    const char *what = "crl_league_create";
    int rc = crl_dev_zalloc(&l->ring, (size_t)num_envs * kRingBytes, what);
    if (!rc) rc = crl_dev_zalloc(&l->assign, (size_t)num_envs * sizeof(int32_t), what);
    if (!rc) rc = crl_dev_zalloc(&l->draw_ctr, (size_t)num_envs * sizeof(uint32_t), what);
    if (!rc) rc = crl_dev_zalloc(&l->ctrl, 3 * kMaxAgents * sizeof(unsigned), what);
    if (rc) {
        crl_league_destroy(l);
        return rc;
    }
    *out = l;
    return CRL_OK;
}

void crl_league_destroy(crl_league *l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    weight_stage_free(l->stage);
    for (int a = 0; a < kMaxAgents; a++) {
        if (l->raw[a]) (void)hipFree(l->raw[a]);
        if (l->T.list[a]) (void)hipFree(l->T.list[a]);
    }
    if (l->act2) (void)hipFree(l->act2);
    if (l->feat) (void)hipFree(l->feat);
    if (l->ring) (void)hipFree(l->ring);
    if (l->assign) (void)hipFree(l->assign);
    if (l->draw_ctr) (void)hipFree(l->draw_ctr);
    if (l->ctrl) (void)hipFree(l->ctrl);
    delete l;
}

int crl_league_add_builtin(crl_league *l, int32_t kind) {
    crl_fail_no_ctx();
    if (!l || (kind != CRL_LEAGUE_RANDOM && kind != CRL_LEAGUE_RULE_BASED))
        return crl_fail(CRL_EINVAL, "crl_league_add_builtin: kind must be CRL_LEAGUE_RANDOM or CRL_LEAGUE_RULE_BASED");
    return league_add(l, kind, nullptr);
}

int crl_league_add_light(crl_league *l, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *actor_w,
                         const float *actor_b) {
    crl_fail_no_ctx();
    if (!l || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b) return crl_fail(CRL_EINVAL, "crl_league_add_light: null argument");
    std::vector<float> raw(kLightRawFloats, 0.f);
    policy_light_pack(raw.data(), conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b);
    return league_add(l, CRL_LEAGUE_LIGHT, raw.data());
}

int crl_pool_add_full(crl_league *l, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *conv3_w,
                      const float *conv3_b, const float *actor_w, const float *actor_b, int64_t scratch_rows) {
    crl_fail_no_ctx();
    if (!l || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !conv3_w || !conv3_b || !actor_w || !actor_b)
        return crl_fail(CRL_EINVAL, "crl_pool_add_full: null argument");
    if (scratch_rows < 0) return crl_fail(CRL_EINVAL, "crl_pool_add_full: scratch_rows must be >= 0 (0: min(num_envs, 65536)), not %lld", (long long)scratch_rows);
    if (l->agents >= kMaxAgents) return crl_fail(CRL_EINVAL, "crl_pool_add_full: at most %d agents in a pool", kMaxAgents);
    if (l->scratch_rows) {
        if (scratch_rows && scratch_rows != l->scratch_rows)
            return crl_fail(CRL_EINVAL, "crl_pool_add_full: scratch_rows %lld, but the league's scratch holds %lld rows (the first full-size agent fixed it; pass 0 or that value)",
                            (long long)scratch_rows, (long long)l->scratch_rows);
        scratch_rows = l->scratch_rows;
    } else if (!scratch_rows) {
        scratch_rows = l->n < 65536 ? l->n : 65536;
    }
    std::vector<float> blob((size_t)policy_full_blob_floats(), 0.f);
    policy_full_pack(blob.data(), conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, actor_w, actor_b);
    return league_add(l, CRL_POOL_KIND_FULL, blob.data(), scratch_rows);
}

// the slot of a reload (`who`): in the pool, and of kind `kind`
static int pool_load_slot(const char *who, crl_league *l, int32_t agent, int kind) {
    if (agent < 0 || agent >= l->agents) return crl_fail(CRL_EINVAL, "%s: agent %d is not in the pool of %d", who, agent, l->agents);
    if (l->kind[agent] != kind)
        return crl_fail(CRL_EINVAL, "%s: agent %d is %s", who, agent,
                        l->kind[agent] == CRL_LEAGUE_LIGHT ? "a LightActorCritic slot (crl_pool_load_light)"
                        : l->kind[agent] == CRL_POOL_KIND_FULL ? "a full-size slot (crl_pool_load_full)" : "a built-in agent without weights");
    return CRL_OK;
}

int crl_pool_load_light(crl_league *l, int32_t agent, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b,
                        const float *actor_w, const float *actor_b, void *stream) {
    crl_fail_no_ctx();
    if (!l || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b) return crl_fail(CRL_EINVAL, "crl_pool_load_light: null argument");
    if (int rc = pool_load_slot("crl_pool_load_light", l, agent, CRL_LEAGUE_LIGHT)) return rc;
    HIP_TRY(hipSetDevice(l->device));
    HIP_TRY(weight_stage_begin(l->stage, kLightRawFloats));
    l->stage.host[kLightRawFloats - 1] = 0.f;  // (the pad behind the actor's bias)
    policy_light_pack(l->stage.host, conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b);
    HIP_TRY(weight_stage_send(l->stage, l->raw[agent], kLightRawFloats, (hipStream_t)stream));
    return CRL_OK;
}

int crl_pool_load_light_dev(crl_league *l, int32_t agent, const float *blob_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !blob_dev) return crl_fail(CRL_EINVAL, "crl_pool_load_light_dev: null argument");
    if (int rc = pool_load_slot("crl_pool_load_light_dev", l, agent, CRL_LEAGUE_LIGHT)) return rc;
    HIP_TRY(hipMemcpyAsync(l->raw[agent], blob_dev, (size_t)kLightRawFloats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_pool_load_full(crl_league *l, int32_t agent, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b,
                       const float *conv3_w, const float *conv3_b, const float *actor_w, const float *actor_b, void *stream) {
    crl_fail_no_ctx();
    if (!l || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !conv3_w || !conv3_b || !actor_w || !actor_b)
        return crl_fail(CRL_EINVAL, "crl_pool_load_full: null argument");
    if (int rc = pool_load_slot("crl_pool_load_full", l, agent, CRL_POOL_KIND_FULL)) return rc;
    const size_t floats = (size_t)policy_full_blob_floats();
    HIP_TRY(hipSetDevice(l->device));
    HIP_TRY(weight_stage_begin(l->stage, floats));
    l->stage.host[floats - 1] = 0.f;  // (the pad behind the actor's bias)
    policy_full_pack(l->stage.host, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, actor_w, actor_b);
    HIP_TRY(weight_stage_send(l->stage, l->raw[agent], floats, (hipStream_t)stream));
    return CRL_OK;
}

int crl_pool_load_full_dev(crl_league *l, int32_t agent, const float *blob_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !blob_dev) return crl_fail(CRL_EINVAL, "crl_pool_load_full_dev: null argument");
    if (int rc = pool_load_slot("crl_pool_load_full_dev", l, agent, CRL_POOL_KIND_FULL)) return rc;
    HIP_TRY(hipMemcpyAsync(l->raw[agent], blob_dev, (size_t)policy_full_blob_floats() * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_pool_get_blob(crl_league *l, int32_t agent, float *blob_out_host, int64_t blob_floats, void *stream) {
    crl_fail_no_ctx();
    if (!l || !blob_out_host) return crl_fail(CRL_EINVAL, "crl_pool_get_blob: null argument");
    if (agent < 0 || agent >= l->agents) return crl_fail(CRL_EINVAL, "crl_pool_get_blob: agent %d is not in the pool of %d", agent, l->agents);
    if (l->kind[agent] != CRL_LEAGUE_LIGHT && l->kind[agent] != CRL_POOL_KIND_FULL)
        return crl_fail(CRL_EINVAL, "crl_pool_get_blob: agent %d is a built-in agent without weights", agent);
    const int64_t floats = l->kind[agent] == CRL_LEAGUE_LIGHT ? (int64_t)kLightRawFloats : policy_full_blob_floats();
    if (blob_floats != floats)
        return crl_fail(CRL_EINVAL, "crl_pool_get_blob: blob_floats %lld, but the slot's blob holds %lld", (long long)blob_floats, (long long)floats);
    HIP_TRY(hipSetDevice(l->device));
    HIP_TRY(hipMemcpyAsync(blob_out_host, l->raw[agent], (size_t)floats * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return CRL_OK;
}

int crl_pool_get_counters(crl_league *l, uint64_t *seed, int64_t *env_id_base, uint32_t *act_calls, uint32_t *draw_ctr_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_pool_get_counters: null pool");
    if (draw_ctr_out_dev)
        HIP_TRY(hipMemcpyAsync(draw_ctr_out_dev, l->draw_ctr, (size_t)l->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (seed) *seed = l->seed;
    if (env_id_base) *env_id_base = l->env_id_base;
    if (act_calls) *act_calls = l->step;
    return CRL_OK;
}

int crl_pool_set_counters(crl_league *l, uint32_t act_calls, const uint32_t *draw_ctr_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_pool_set_counters: null pool");
    if (draw_ctr_dev)
        HIP_TRY(hipMemcpyAsync(l->draw_ctr, draw_ctr_dev, (size_t)l->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    l->step = act_calls;
    return CRL_OK;
}

int crl_sampling_set_agent(crl_league *l, int32_t agent, float temperature, float epsilon) {
    crl_fail_no_ctx();
    SampleArgs S{};
    if (int rc = sample_args_from(temperature, epsilon, "crl_sampling_set_agent", &S)) return rc;
    if (!l) return crl_fail(CRL_EINVAL, "crl_sampling_set_agent: null league");
    if (agent < 0 || agent >= l->agents) return crl_fail(CRL_EINVAL, "crl_sampling_set_agent: agent %d is not in the pool of %d", agent, l->agents);
    l->temperature[agent] = temperature, l->epsilon[agent] = epsilon, l->sample[agent] = S;
    return CRL_OK;
}

int crl_sampling_get_agent(crl_league *l, int32_t agent, float *temperature, float *epsilon) {
    crl_fail_no_ctx();
    if (!l || !temperature || !epsilon) return crl_fail(CRL_EINVAL, "crl_sampling_get_agent: null argument");
    if (agent < 0 || agent >= l->agents) return crl_fail(CRL_EINVAL, "crl_sampling_get_agent: agent %d is not in the pool of %d", agent, l->agents);
    *temperature = l->temperature[agent], *epsilon = l->epsilon[agent];
    return CRL_OK;
}

int crl_league_seed(crl_league *l, uint64_t seed, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_league_seed: null league");
    HIP_TRY(hipMemsetAsync(l->draw_ctr, 0, (size_t)l->n * sizeof(uint32_t), (hipStream_t)stream));
    l->seed = seed, l->step = 0;
    return CRL_OK;
}

int crl_league_set_assignment(crl_league *l, const int32_t *ids_dev, int32_t all, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_league_set_assignment: null league");
    hipStream_t st = (hipStream_t)stream;
    if (ids_dev) {
        HIP_TRY(hipMemcpyAsync(l->assign, ids_dev, (size_t)l->n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    } else {
        if (all < 0 || all >= l->agents) return crl_fail(CRL_EINVAL, "crl_league_set_assignment: agent %d is not in the pool of %d", all, l->agents);
        hipLaunchKernelGGL(league_fill_assignment_kernel, dim3((unsigned)((l->n + 255) / 256)), dim3(256), 0, st, l->assign, all, l->n);
        HIP_TRY(hipGetLastError());
    }
    return league_partition(l, nullptr, 0, st);
}

int crl_league_get_assignment(crl_league *l, int32_t *ids_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !ids_out_dev) return crl_fail(CRL_EINVAL, "crl_league_get_assignment: null argument");
    HIP_TRY(hipMemcpyAsync(ids_out_dev, l->assign, (size_t)l->n * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_league_resample(crl_league *l, const uint8_t *done_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_league_resample: null league");
    return league_partition(l, done_dev, done_dev == nullptr, (hipStream_t)stream);
}

int crl_league_get_lists(crl_league *l, int32_t *counts_out_dev, int32_t *lists_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!l || !counts_out_dev) return crl_fail(CRL_EINVAL, "crl_league_get_lists: null argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(counts_out_dev, league_counts(l), kMaxAgents * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (lists_out_dev)
        for (int a = 0; a < l->agents; a++)
            if (l->T.list[a])
                HIP_TRY(hipMemcpyAsync(lists_out_dev + (int64_t)a * l->n, l->T.list[a], (size_t)l->n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return CRL_OK;
}

int crl_league_act(crl_league *l, const uint8_t *frame_dev, int64_t frame_stride, int32_t *actions_dev, int64_t action_stride, float *logits_dev,
                   void *stream) {
    crl_fail_no_ctx();
    if (!l || !frame_dev || !actions_dev) return crl_fail(CRL_EINVAL, "crl_league_act: null argument");
    if (int rc = ring_check_act("crl_league_act", frame_dev, frame_stride, action_stride)) return rc;
    if (l->agents <= 0) return crl_fail(CRL_ESTATE, "crl_league_act: the pool is empty");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(l->ctrl, 0, kMaxAgents * sizeof(unsigned), st));  // the tickets
    LeagueExplore E{};
    for (int a = 0; a < l->agents; a++)
        if (l->kind[a] == CRL_LEAGUE_RULE_BASED) E.eps_q[a] = l->sample[a].eps_q;
    hipLaunchKernelGGL(league_fill_kernel, dim3((unsigned)((l->n + kLThreads - 1) / kLThreads)), dim3(kLThreads), 0, st, league_kinds(l), l->agents,
                       l->assign, l->ring, l->head, frame_dev, frame_stride, actions_dev, action_stride, l->seed, l->env_id_base, l->step, l->n, E);
    HIP_TRY(hipGetLastError());
    for (int a = 0; a < l->agents; a++) {
        if (l->kind[a] != CRL_LEAGUE_LIGHT && l->kind[a] != CRL_POOL_KIND_FULL) continue;
        SampleArgs S = l->sample[a];  // an agent at (0, 0) -- every agent, until crl_sampling_set_agent -- keeps the greedy launch
        const SampleArgs *sample = sample_active(S) ? &S : nullptr;
        S.seed = l->seed, S.id_base = l->env_id_base, S.n = l->step;
        if (l->kind[a] == CRL_LEAGUE_LIGHT)
            HIP_TRY(policy_light_act_list(l->raw[a], l->ring, l->head, frame_dev, frame_stride, actions_dev, action_stride, logits_dev, l->T.list[a],
                                          league_counts(l) + a, l->n, l->cus, l->ctrl + a, sample, st));
        else
            HIP_TRY(policy_full_act_list(l->raw[a], l->act2, l->feat, l->scratch_rows, l->ring, l->head, frame_dev, frame_stride, actions_dev, action_stride,
                                         logits_dev, l->T.list[a], league_counts(l) + a, l->n, l->cus, sample, st));
    }
    l->head = (l->head + 1) & 3;
    l->step++;
    return CRL_OK;
}

int crl_league_reset(crl_league *l, void *stream) {
    crl_fail_no_ctx();
    if (!l) return crl_fail(CRL_EINVAL, "crl_league_reset: null league");
    HIP_TRY(ring_reset(l->ring, l->n, (hipStream_t)stream));
    l->head = 0;
    return CRL_OK;
}

int crl_league_get_stack(crl_league *l, uint8_t *stack_out_dev, void *stream) { return ring_copy_stack("crl_league_get_stack", l, stack_out_dev, 0, stream); }
int crl_league_set_stack(crl_league *l, const uint8_t *stack_in_dev, void *stream) { return ring_copy_stack("crl_league_set_stack", l, stack_in_dev, 1, stream); }

}  // extern "C"

// car_policy.hip -- the learned CarRacing drivers (include/crl.h "car policy"): a 21-float state observation per car, computed from the
// env's committed device state, and the reference's MLP (utils/network.py:59-70: fc1 -> 100, ReLU, policy, value) on it, served per env
// and per car from CRL_CAR_POLICY_SLOTS weight sets, with Gaussian actions, values and log-probabilities.  An object beside a
// CarRacing context, as crl_car_driver is: it reads the context's state and writes the caller's tensors.
//
// One launch per act / observe call: ONE WAVEFRONT PER ENV, as car_driver_kernel.  The nearest-tile search runs once for both cars
// (car_search.h).  The features are wave-uniform arithmetic: every lane holds all 21.  The network spreads the 100 hidden units over
// the lanes -- lane L owns units L and, for L < 36, L + 64 -- and reads the slot's blob with the lane index innermost (fc1_w is stored
// transposed: input k's 100 weights lie side by side), so a wave's load of one input's weights is 400 contiguous bytes; the three
// 100-term output sums are one product (or two) per lane and six butterfly steps of cross-lane moves.  The draw is wave-uniform but for
// the Box-Muller transform, which lane d evaluates for component d.  No LDS, no barrier; lane 0 stores the car's scalars, lanes 0..20
// its observation.
#include <math.h>

#include "car_device.h"
#include "car_search.h"
#include "crl_internal.h"
#include "crl_rot.h"

#pragma clang fp contract(off)

namespace crl {

static constexpr int kPolicyWaves = 4;  // envs per workgroup
static constexpr int kHid = CRL_CAR_POLICY_HIDDEN, kFeat = CRL_CAR_OBS_FEATURES, kBlob = CRL_CAR_POLICY_BLOB_FLOATS;
// offsets into a slot's blob (include/crl.h)
static constexpr int kOffB1 = kFeat * kHid, kOffPol = kOffB1 + kHid, kOffVal = kOffPol + 2 * kHid, kOffTail = kOffVal + kHid;
static_assert(kOffTail + 8 == kBlob && kHid > 64 && kHid <= 128, "blob layout of include/crl.h \"car policy\"");

// what a launch carries
struct PolicyArgs {
    const float *body;            // [30][M]
    const int32_t *done;          // [M]
    const int32_t *visited_count; // [M]
    const int16_t *wtiles;        // [4][kWheelSlots][M]
    const int32_t *ntiles;        // [n]
    const float4 *tile_aabb_em;   // [n][512]
    const int32_t *assign;        // [n][players]; nullptr: observe only, no network runs
    const float *blobs;           // [CRL_CAR_POLICY_SLOTS][kBlob]
    float *actions, *values, *logp, *noise, *obs;  // all but the one a call is about are optional
    int64_t n;
    int32_t players;
    uint32_t call;
    uint64_t seed;
    int64_t id_base;
    int8_t flag[CRL_CAR_POLICY_SLOTS];  // -1 = empty slot, 0 = sampling, 1 = deterministic
};

// the wave's sum of p in the written order: p_L + p_{L xor m} for m = 32, 16, .., 1
__device__ __forceinline__ float wave_sum_butterfly(float p) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_xor(p, m, 64);
    return p;
}

// one car of one env, after the search: its features, its network, its draw, its stores
__device__ __forceinline__ void policy_car(const PolicyArgs &A, int64_t env, int n, int c, int slot, bool live, int nearest,
                                           const float4 *__restrict__ boxes, int lane) {
    const int64_t M = A.n * A.players, ci = (int64_t)c * A.n + env, row = env * A.players + c;
    const bool served = slot >= 0;
    float x[kFeat];
#pragma unroll
    for (int k = 0; k < kFeat; k++) x[k] = 0.f;
    if (live && (served || A.obs)) {
        const float *__restrict__ B = A.body + ci;
        const float cx = B[0 * M], cy = B[1 * M], a = B[2 * M], vx = B[3 * M], vy = B[4 * M], w = B[5 * M];
        // wheel k's body: rows 6 + 6 k (cx), 7 + 6 k (cy), 8 + 6 k (angle)
        const float w0x = B[6 * M], w0y = B[7 * M], w0a = B[8 * M], w1x = B[12 * M], w1y = B[13 * M];
        const float w2x = B[18 * M], w2y = B[19 * M], w3x = B[24 * M], w3y = B[25 * M];
        const float hx = (w0x + w1x) * 0.5f - (w2x + w3x) * 0.5f, hy = (w0y + w1y) * 0.5f - (w2y + w3y) * 0.5f;
        const float len = sqrtf(hx * hx + hy * hy);
        float fx = 1.f, fy = 0.f;
        if (len > 0.f) fx = hx / len, fy = hy / len;
        const float lx = -fy, ly = fx;
#define CAR_FRAME(px, py, k, scale) (x[k] = ((px) * fx + (py) * fy) * (scale), x[(k) + 1] = ((px) * lx + (py) * ly) * (scale))
        CAR_FRAME(vx, vy, 0, CRL_CAR_OBS_SPEED_SCALE);
        x[2] = w * 0.25f;
        x[3] = (w0a - a) * 2.0f;
        // lane 6 w + k looks at slot k of wheel w
        const bool touch = lane < 4 * kWheelSlots && A.wtiles[(int64_t)lane * M + ci] >= 0;
        const unsigned long long tb = __ballot(touch);
        int wheels = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) wheels += ((tb >> (kWheelSlots * k)) & ((1u << kWheelSlots) - 1u)) != 0;
        x[4] = (float)wheels * 0.25f;
        x[5] = (float)A.visited_count[ci] / (float)n;
#pragma unroll
        for (int m = 0; m < 5; m++) {
            const int g = (nearest + (m == 0 ? 0 : 1 << m)) % n;  // offsets 0, 2, 4, 8, 16
            const float4 b = boxes[g];
            const float ax = (b.x + b.z) * 0.5f - cx, ay = (b.y + b.w) * 0.5f - cy;
            CAR_FRAME(ax, ay, 6 + 2 * m, CRL_CAR_OBS_DIST_SCALE);
        }
        if (A.players == 2) {
            const int64_t oi = (int64_t)(1 - c) * A.n + env;
            const float *__restrict__ O = A.body + oi;
            const float px = O[0 * M] - cx, py = O[1 * M] - cy, qx = O[3 * M] - vx, qy = O[4 * M] - vy;
            CAR_FRAME(px, py, 16, CRL_CAR_OBS_DIST_SCALE);
            CAR_FRAME(qx, qy, 18, CRL_CAR_OBS_SPEED_SCALE);
            x[20] = A.done[oi] == 0 ? 1.f : 0.f;
        }
#undef CAR_FRAME
    }
    if (A.obs) {
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < kFeat; k++) mine = lane == k ? x[k] : mine;
        if (lane < kFeat) A.obs[row * kFeat + lane] = mine;
    }

    float u0 = 0.f, u1 = 0.f, value = 0.f, lp = 0.f, z0 = 0.f, z1 = 0.f;
    if (served && live) {
        const float *__restrict__ W = A.blobs + (int64_t)slot * kBlob;
        const bool two = lane < kHid - 64;
        const int j0 = lane, j1 = two ? lane + 64 : lane;  // (a lane without a second unit reads its first again and drops it)
        float a0 = W[kOffB1 + j0], a1 = W[kOffB1 + j1];
#pragma unroll
        for (int k = 0; k < kFeat; k++) {
            a0 = a0 + W[k * kHid + j0] * x[k];
            a1 = a1 + W[k * kHid + j1] * x[k];
        }
        const float h0 = a0 > 0.f ? a0 : 0.f, h1 = a1 > 0.f ? a1 : 0.f;
        float out[3];
#pragma unroll
        for (int o = 0; o < 3; o++) {
            const float *__restrict__ r = W + kOffPol + o * kHid;  // policy_w[0], policy_w[1], value_w[0]
            float p = h0 * r[j0];
            const float q = p + h1 * r[j1];
            p = two ? q : p;
            out[o] = wave_sum_butterfly(p) + W[kOffTail + o];
        }
        value = out[2];
        if (A.flag[slot] != 0) u0 = out[0], u1 = out[1];
        else {
            const float ls0 = W[kOffTail + 3], ls1 = W[kOffTail + 4], sd0 = W[kOffTail + 5], sd1 = W[kOffTail + 6];
            const uint64_t gid = (uint64_t)(A.id_base + env);
            uint32_t r[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), A.call, CRL_CAR_POLICY_DOMAIN + (uint32_t)c};
            driver_philox(r, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
            // lane d evaluates component d (the other lanes repeat one of the two)
            const bool second = (lane & 1) != 0;
            const uint32_t ra = second ? r[2] : r[0], rb = second ? r[3] : r[1];
            const float v1 = (float)((ra >> 8) + 1u) * 0x1p-24f, v2 = (float)(rb >> 8) * 0x1p-24f;
            const float rad = sqrtf(-2.0f * logf(v1));
            float sn, cs;
            crl_sincosf(CRL_CAR_POLICY_TWO_PI * v2, &sn, &cs);
            const float z = rad * cs;
            z0 = __shfl(z, 0, 64), z1 = __shfl(z, 1, 64);
            u0 = out[0] + sd0 * z0, u1 = out[1] + sd1 * z1;
            lp = (((-0.5f * z0) * z0 - ls0) + ((-0.5f * z1) * z1 - ls1)) - CRL_CAR_POLICY_LN_2PI;
        }
    }
    if (lane == 0) {
        if (served) A.actions[row * 2] = u0, A.actions[row * 2 + 1] = u1;
        if (A.values) A.values[row] = value;
        if (A.logp) A.logp[row] = lp;
        if (A.noise) A.noise[row * 2] = z0, A.noise[row * 2 + 1] = z1;
    }
}

__global__ __launch_bounds__(64 * kPolicyWaves) void car_policy_kernel(const PolicyArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t env = (int64_t)blockIdx.x * kPolicyWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (env >= A.n) return;
    const int n = min(A.ntiles[env], kCarMaxTiles);
    const int64_t M = A.n * A.players;
    int slot[2] = {-1, -1};
    bool live[2] = {false, false};
    float cx[2] = {0.f, 0.f}, cy[2] = {0.f, 0.f};
    bool search = false;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (c >= A.players) continue;
        const int64_t ci = (int64_t)c * A.n + env;
        if (A.assign) {
            const int32_t id = A.assign[env * A.players + c];
            if (id >= 0 && id < CRL_CAR_POLICY_SLOTS && A.flag[id] >= 0) slot[c] = id;
        }
        live[c] = A.done[ci] == 0 && n > 0;
        if (live[c] && (slot[c] >= 0 || A.obs)) cx[c] = A.body[0 * M + ci], cy[c] = A.body[1 * M + ci], search = true;
    }
    int near0 = 0, near1 = 0;
    const float4 *__restrict__ boxes = A.tile_aabb_em + env * kCarMaxTiles;
    if (search) car_nearest2(boxes, n, lane, cx[0], cy[0], cx[1], cy[1], near0, near1);
    policy_car(A, env, n, 0, slot[0], live[0], near0, boxes, lane);
    if (A.players == 2) policy_car(A, env, n, 1, slot[1], live[1], near1, boxes, lane);
}

}  // namespace crl

using namespace crl;

struct crl_car_policy {
    crl_car_ctx *car = nullptr;
    int64_t n = 0;
    int players = 0;
    int64_t id_base = 0;
    uint64_t seed = 0;
    uint32_t calls = 0;
    int32_t *assign = nullptr;  // [n][players] on the device
    float *blobs = nullptr;     // [CRL_CAR_POLICY_SLOTS][kBlob] on the device
    int8_t flag[CRL_CAR_POLICY_SLOTS];
};

crl_car_ctx *crl_car_policy_ctx(crl_car_policy *p) { return p->car; }
int32_t *crl_car_policy_assign_dev(crl_car_policy *p) { return p->assign; }

static int policy_launch(crl_car_policy *p, bool act, float *actions, float *values, float *logp, float *noise, float *obs, void *stream) {
    const CarSoA *s = crl_car_soa(p->car);
    PolicyArgs A;
    A.body = s->body, A.done = s->done, A.visited_count = s->visited_count, A.wtiles = s->wtiles, A.ntiles = s->ntiles;
    A.tile_aabb_em = s->tile_aabb_em, A.assign = act ? p->assign : nullptr, A.blobs = p->blobs;
    A.actions = actions, A.values = values, A.logp = logp, A.noise = noise, A.obs = obs;
    A.n = p->n, A.players = p->players, A.call = p->calls, A.seed = p->seed, A.id_base = p->id_base;
    for (int k = 0; k < CRL_CAR_POLICY_SLOTS; k++) A.flag[k] = p->flag[k];
    const unsigned blocks = (unsigned)((p->n + kPolicyWaves - 1) / kPolicyWaves);
    hipLaunchKernelGGL(car_policy_kernel, dim3(blocks), dim3(64 * kPolicyWaves), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return CRL_OK;
}

static int policy_slot_ok(const char *fn, int32_t slot) {
    if (slot < 0 || slot >= CRL_CAR_POLICY_SLOTS) return crl_fail(CRL_EINVAL, "%s: slot %d lies outside [0, %d)", fn, slot, CRL_CAR_POLICY_SLOTS);
    return CRL_OK;
}

static int policy_flag_ok(const char *fn, int32_t deterministic) {
    if (deterministic != 0 && deterministic != 1) return crl_fail(CRL_EINVAL, "%s: deterministic must be 0 or 1, not %d", fn, deterministic);
    return CRL_OK;
}

extern "C" {

int crl_car_policy_create(crl_ctx *ctx, uint64_t seed, crl_car_policy **out) {
    crl_fail_no_ctx();
    if (!ctx || !out) return crl_fail(CRL_EINVAL, "crl_car_policy_create: null argument");
    crl_car_ctx *car = crl_ctx_car(ctx);
    if (!car) return crl_fail(CRL_EINVAL, "crl_car_policy_create: not a CarRacing context");
    const CarSoA *s = crl_car_soa(car);
    crl_car_policy *p = new crl_car_policy();
    p->car = car, p->n = s->n, p->players = s->players, p->id_base = crl_car_env_id_base(car), p->seed = seed;
    for (int k = 0; k < CRL_CAR_POLICY_SLOTS; k++) p->flag[k] = -1;
    const size_t bytes = (size_t)p->n * p->players * sizeof(int32_t);
    hipError_t e = hipMalloc((void **)&p->assign, bytes);
    if (e == hipSuccess) e = hipMemset(p->assign, 0xFF, bytes);  // -1: nobody is served until assigned
    int rc = e == hipSuccess ? CRL_OK : crl_hip_fail(e, "crl_car_policy_create");
    if (rc == CRL_OK) rc = crl_dev_zalloc(&p->blobs, (size_t)CRL_CAR_POLICY_SLOTS * kBlob * sizeof(float), "crl_car_policy_create");
    if (rc != CRL_OK) {
        crl_car_policy_destroy(p);
        return rc;
    }
    *out = p;
    return CRL_OK;
}

void crl_car_policy_destroy(crl_car_policy *p) {
    if (!p) return;
    if (p->assign) (void)hipFree(p->assign);
    if (p->blobs) (void)hipFree(p->blobs);
    delete p;
}

int crl_car_policy_set_weights(crl_car_policy *p, int32_t slot, const float *blob, int32_t deterministic, void *stream) {
    crl_fail_no_ctx();
    if (int rc = policy_slot_ok("crl_car_policy_set_weights", slot)) return rc;
    if (int rc = policy_flag_ok("crl_car_policy_set_weights", deterministic)) return rc;
    if (!p || !blob) return crl_fail(CRL_EINVAL, "crl_car_policy_set_weights: null argument");
    HIP_TRY(hipMemcpyAsync(p->blobs + (size_t)slot * kBlob, blob, kBlob * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
    p->flag[slot] = (int8_t)deterministic;
    return CRL_OK;
}

int crl_car_policy_get_weights(crl_car_policy *p, int32_t slot, float *blob_out, int32_t *deterministic_out, void *stream) {
    crl_fail_no_ctx();
    if (int rc = policy_slot_ok("crl_car_policy_get_weights", slot)) return rc;
    if (!p) return crl_fail(CRL_EINVAL, "crl_car_policy_get_weights: null policy");
    if (p->flag[slot] < 0) return crl_fail(CRL_EINVAL, "crl_car_policy_get_weights: slot %d is empty", slot);
    if (blob_out) HIP_TRY(hipMemcpyAsync(blob_out, p->blobs + (size_t)slot * kBlob, kBlob * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
    if (deterministic_out) *deterministic_out = p->flag[slot];
    return CRL_OK;
}

int crl_car_policy_set_sampling(crl_car_policy *p, int32_t slot, int32_t deterministic) {
    crl_fail_no_ctx();
    if (int rc = policy_slot_ok("crl_car_policy_set_sampling", slot)) return rc;
    if (int rc = policy_flag_ok("crl_car_policy_set_sampling", deterministic)) return rc;
    if (!p) return crl_fail(CRL_EINVAL, "crl_car_policy_set_sampling: null policy");
    if (p->flag[slot] < 0) return crl_fail(CRL_EINVAL, "crl_car_policy_set_sampling: slot %d is empty", slot);
    p->flag[slot] = (int8_t)deterministic;
    return CRL_OK;
}

int crl_car_policy_set_assignment(crl_car_policy *p, const int32_t *ids_dev, void *stream) {
    crl_fail_no_ctx();
    if (!p || !ids_dev) return crl_fail(CRL_EINVAL, "crl_car_policy_set_assignment: null argument");
    HIP_TRY(hipMemcpyAsync(p->assign, ids_dev, (size_t)p->n * p->players * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_car_policy_get_assignment(crl_car_policy *p, int32_t *ids_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!p || !ids_out_dev) return crl_fail(CRL_EINVAL, "crl_car_policy_get_assignment: null argument");
    HIP_TRY(hipMemcpyAsync(ids_out_dev, p->assign, (size_t)p->n * p->players * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_car_policy_act(crl_car_policy *p, float *actions_dev, float *values_dev, float *log_probs_dev, float *noise_dev, float *obs_dev,
                       void *stream) {
    crl_fail_no_ctx();
    if (!p || !actions_dev) return crl_fail(CRL_EINVAL, "crl_car_policy_act: null argument");
    if (int rc = policy_launch(p, true, actions_dev, values_dev, log_probs_dev, noise_dev, obs_dev, stream)) return rc;
    p->calls++;
    return CRL_OK;
}

int crl_car_policy_observe(crl_car_policy *p, float *obs_dev, void *stream) {
    crl_fail_no_ctx();
    if (!p || !obs_dev) return crl_fail(CRL_EINVAL, "crl_car_policy_observe: null argument");
    return policy_launch(p, false, nullptr, nullptr, nullptr, nullptr, obs_dev, stream);
}

int crl_car_policy_get_counters(crl_car_policy *p, uint64_t *seed, int64_t *calls) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_car_policy_get_counters: null policy");
    if (seed) *seed = p->seed;
    if (calls) *calls = (int64_t)p->calls;
    return CRL_OK;
}

int crl_car_policy_set_counters(crl_car_policy *p, uint64_t seed, int64_t calls) {
    crl_fail_no_ctx();
    if (calls < 0 || calls > 0xFFFFFFFFll) return crl_fail(CRL_EINVAL, "crl_car_policy_set_counters: calls must lie in [0, 2^32), not %lld", (long long)calls);
    if (!p) return crl_fail(CRL_EINVAL, "crl_car_policy_set_counters: null policy");
    p->seed = seed, p->calls = (uint32_t)calls;
    return CRL_OK;
}

}  // extern "C"

// car_driver.hip -- the built-in CarRacing agents (include/crl.h "car drivers"): RANDOM and the track-following RULE_BASED driver,
// served per env and per car from the env's own device state.  An object beside a CarRacing context, as the ledger is beside the
// league: it reads the context's committed state (bodies, done flags, tile count, the env-major tile boxes) and writes the
// caller's action tensor; nothing here reaches into the step pipeline.
//
// Stands in for the opponent_policy a caller hands to make_competitive_car_racing (car_racing/make_competitive_car_racing.py:10-58;
// the reference ships none) and is CarRacing's counterpart of pong/builtin_policies.py:44-58.
//
// One launch per act call: ONE WAVEFRONT PER ENV.  The 64 lanes walk the env's n <= 512 boxes of tile_aabb_em ([n][512] float4: 16
// bytes per lane, 1 KiB per load, at most 8 loads), each box read once for both cars (car_search.h: car_nearest2).  No LDS, no barrier.
// What follows the search is wave-uniform arithmetic; lane 0 stores the car's two floats.
#include <math.h>

#include "car_device.h"
#include "car_search.h"
#include "crl_internal.h"

#pragma clang fp contract(off)

namespace crl {

struct DriverStyle {
    int32_t kind;  // crl_car_driver_kind, -1 = empty slot
    float target_speed;
    int32_t lookahead;
    float steer_gain;
    uint32_t eps_q;  // min(floor(epsilon * 2^32), 0xFFFFFFFF)
};

// what a launch carries (kernel arguments: the styles travel with it, nothing of them lives in device memory)
struct DriverArgs {
    const float *body;           // [30][M]
    const int32_t *done;         // [M]
    const int32_t *ntiles;       // [n]
    const float4 *tile_aabb_em;  // [n][512]
    const int32_t *assign;       // [n][players]
    int64_t n;
    int32_t players;
    uint32_t call;
    uint64_t seed;
    int64_t id_base;
    DriverStyle style[CRL_CAR_DRIVER_SLOTS];
};

__device__ inline float driver_unit(uint32_t x) { return (float)((int32_t)(x >> 8) - 8388608) * 0x1p-23f; }
__device__ inline float driver_clamp(float x) { return x < -1.0f ? -1.0f : x > 1.0f ? 1.0f : x; }

static constexpr int kDriverWaves = 4;  // envs per workgroup

// what the wave knows of one car before the search (wave-uniform)
struct DriverPlan {
    bool served = false;  // assigned to a style that exists: its two floats are written
    bool random = false;  // ... with the draw's action
    bool search = false;  // ... with the rule's: needs the nearest tile
    float cx = 0.f, cy = 0.f, rx = 0.f, ry = 0.f;
    DriverStyle S = {-1, 0.f, 0, 0.f, 0u};
};

__device__ __forceinline__ DriverPlan driver_plan(const DriverArgs &A, int64_t env, int n, int c) {
    DriverPlan P;
    if (c >= A.players) return P;
    const int32_t id = A.assign[env * A.players + c];
    if (id < 0 || id >= CRL_CAR_DRIVER_SLOTS) return P;
    P.S = A.style[id];
    if (P.S.kind < 0) return P;
    P.served = true;
    const int64_t M = A.n * A.players, ci = (int64_t)c * A.n + env;
    if (A.done[ci] != 0 || n <= 0) return P;  // rule 0: (0, 0)
    const uint64_t gid = (uint64_t)(A.id_base + env);
    uint32_t x[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), A.call, CRL_CAR_DRIVER_DOMAIN + (uint32_t)c};
    driver_philox(x, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));  // rule 1
    P.rx = driver_unit(x[0]), P.ry = driver_unit(x[1]);
    P.random = P.S.kind == CRL_CAR_DRIVER_RANDOM || x[2] < P.S.eps_q;
    P.search = !P.random;
    P.cx = A.body[0 * M + ci], P.cy = A.body[1 * M + ci];
    return P;
}

// rules 3-6 for a car whose nearest tile is known, and the store of its action by lane 0
__device__ __forceinline__ void driver_finish(const DriverArgs &A, const DriverPlan &P, int64_t env, int n, int c, int nearest,
                                              const float4 *__restrict__ boxes, int lane, float *__restrict__ actions) {
    if (!P.served) return;
    float steer = 0.f, gas = 0.f;
    if (P.random) steer = P.rx, gas = P.ry;
    else if (P.search) {
        const int64_t M = A.n * A.players;
        const float *__restrict__ B = A.body + ((int64_t)c * A.n + env);
        const float vx = B[3 * M], vy = B[4 * M];
        // wheel k's body: rows 6 + 6 k (cx), 7 + 6 k (cy)
        const float w0x = B[6 * M], w0y = B[7 * M], w1x = B[12 * M], w1y = B[13 * M];
        const float w2x = B[18 * M], w2y = B[19 * M], w3x = B[24 * M], w3y = B[25 * M];
        const int g = (nearest + P.S.lookahead) % n;  // rule 3
        const float4 b = boxes[g];
        const float ax = (b.x + b.z) * 0.5f - P.cx, ay = (b.y + b.w) * 0.5f - P.cy;
        const float hx = (w0x + w1x) * 0.5f - (w2x + w3x) * 0.5f, hy = (w0y + w1y) * 0.5f - (w2y + w3y) * 0.5f;  // rule 4
        const float cr = hx * ay - hy * ax, dt = hx * ax + hy * ay;
        const float den = sqrtf(hx * hx + hy * hy) * sqrtf(ax * ax + ay * ay);
        float sn = 0.f, cs = 1.f;
        if (den > 0.f) sn = cr / den, cs = dt / den;
        const float e = cs >= 0.f ? sn : sn > 0.f ? 1.f : sn < 0.f ? -1.f : 0.f;
        steer = driver_clamp(-(P.S.steer_gain * e));  // rule 5
        const float v = sqrtf(vx * vx + vy * vy);    // rule 6
        const float want = P.S.target_speed * (1.0f - CRL_CAR_DRIVER_CURVE_SLOW * fabsf(e));
        gas = driver_clamp((want - v) * CRL_CAR_DRIVER_GAS_GAIN);
    }
    if (lane == 0) {
        float *out = actions + (env * A.players + c) * 2;
        out[0] = steer, out[1] = gas;
    }
}

__global__ __launch_bounds__(64 * kDriverWaves) void car_driver_kernel(const DriverArgs A, float *__restrict__ actions) {
    const int lane = threadIdx.x & 63;
    const int64_t env = (int64_t)blockIdx.x * kDriverWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (env >= A.n) return;
    const int n = min(A.ntiles[env], kCarMaxTiles);
    const DriverPlan P0 = driver_plan(A, env, n, 0), P1 = driver_plan(A, env, n, 1);

    // rule 2: the nearest tile of each car that needs one
    int near0 = 0, near1 = 0;
    const float4 *__restrict__ boxes = A.tile_aabb_em + env * kCarMaxTiles;
    if (P0.search || P1.search) car_nearest2(boxes, n, lane, P0.cx, P0.cy, P1.cx, P1.cy, near0, near1);
    driver_finish(A, P0, env, n, 0, near0, boxes, lane, actions);
    driver_finish(A, P1, env, n, 1, near1, boxes, lane, actions);
}

}  // namespace crl

using namespace crl;

struct crl_car_driver {
    crl_car_ctx *car = nullptr;
    int64_t n = 0;
    int players = 0;
    int64_t id_base = 0;
    uint64_t seed = 0;
    uint32_t calls = 0;
    int32_t *assign = nullptr;  // [n][players] on the device
    DriverStyle style[CRL_CAR_DRIVER_SLOTS];
    float epsilon[CRL_CAR_DRIVER_SLOTS];
};

crl_car_ctx *crl_car_driver_ctx(crl_car_driver *d) { return d->car; }
int32_t *crl_car_driver_assign_dev(crl_car_driver *d) { return d->assign; }

static uint32_t driver_eps_q(float epsilon) {
    const double q = floor((double)epsilon * 4294967296.0);
    return q >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)q;
}

extern "C" {

int crl_car_driver_create(crl_ctx *ctx, uint64_t seed, crl_car_driver **out) {
    crl_fail_no_ctx();
    if (!ctx || !out) return crl_fail(CRL_EINVAL, "crl_car_driver_create: null argument");
    crl_car_ctx *car = crl_ctx_car(ctx);
    if (!car) return crl_fail(CRL_EINVAL, "crl_car_driver_create: not a CarRacing context");
    const CarSoA *s = crl_car_soa(car);
    crl_car_driver *d = new crl_car_driver();
    d->car = car, d->n = s->n, d->players = s->players, d->id_base = crl_car_env_id_base(car), d->seed = seed;
    for (int k = 0; k < CRL_CAR_DRIVER_SLOTS; k++) d->style[k] = DriverStyle{-1, 0.f, 0, 0.f, 0u}, d->epsilon[k] = 0.f;
    d->style[0] = DriverStyle{CRL_CAR_DRIVER_RANDOM, 0.f, 0, 0.f, 0u};
    d->style[1] = DriverStyle{CRL_CAR_DRIVER_RULE_BASED, CRL_CAR_DRIVER_DEFAULT_TARGET_SPEED, CRL_CAR_DRIVER_DEFAULT_LOOKAHEAD,
                              CRL_CAR_DRIVER_DEFAULT_STEER_GAIN, 0u};
    const size_t bytes = (size_t)d->n * d->players * sizeof(int32_t);
    hipError_t e = hipMalloc((void **)&d->assign, bytes);
    if (e == hipSuccess) e = hipMemset(d->assign, 0xFF, bytes);  // -1: nobody is driven until assigned
    if (e != hipSuccess) {
        if (d->assign) (void)hipFree(d->assign);
        delete d;
        return crl_hip_fail(e, "crl_car_driver_create");
    }
    *out = d;
    return CRL_OK;
}

void crl_car_driver_destroy(crl_car_driver *d) {
    if (!d) return;
    if (d->assign) (void)hipFree(d->assign);
    delete d;
}

int crl_car_driver_set_style(crl_car_driver *d, int32_t slot, int32_t kind, float target_speed, int32_t lookahead, float steer_gain,
                             float epsilon) {
    crl_fail_no_ctx();
    if (slot < 0 || slot >= CRL_CAR_DRIVER_SLOTS) return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: slot %d lies outside [0, %d)", slot, CRL_CAR_DRIVER_SLOTS);
    if (kind != CRL_CAR_DRIVER_RANDOM && kind != CRL_CAR_DRIVER_RULE_BASED)
        return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: kind must be CRL_CAR_DRIVER_RANDOM or CRL_CAR_DRIVER_RULE_BASED, not %d", kind);
    if (!isfinite(target_speed) || !(target_speed >= 0.f))
        return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: target_speed must be finite and >= 0, not %g", (double)target_speed);
    if (lookahead < 0 || lookahead > CRL_CAR_DRIVER_MAX_LOOKAHEAD)
        return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: lookahead must lie in [0, %d], not %d", CRL_CAR_DRIVER_MAX_LOOKAHEAD, lookahead);
    if (!isfinite(steer_gain) || !(steer_gain >= 0.f))
        return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: steer_gain must be finite and >= 0, not %g", (double)steer_gain);
    if (!(epsilon >= 0.f && epsilon <= 1.f)) return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: epsilon must lie in [0, 1], not %g", (double)epsilon);
    if (!d) return crl_fail(CRL_EINVAL, "crl_car_driver_set_style: null driver");
    d->style[slot] = DriverStyle{kind, target_speed, lookahead, steer_gain, driver_eps_q(epsilon)};
    d->epsilon[slot] = epsilon;
    return CRL_OK;
}

int crl_car_driver_get_style(crl_car_driver *d, int32_t slot, int32_t *kind, float *target_speed, int32_t *lookahead, float *steer_gain,
                             float *epsilon) {
    crl_fail_no_ctx();
    if (slot < 0 || slot >= CRL_CAR_DRIVER_SLOTS) return crl_fail(CRL_EINVAL, "crl_car_driver_get_style: slot %d lies outside [0, %d)", slot, CRL_CAR_DRIVER_SLOTS);
    if (!d) return crl_fail(CRL_EINVAL, "crl_car_driver_get_style: null driver");
    const DriverStyle &s = d->style[slot];
    if (kind) *kind = s.kind;
    if (target_speed) *target_speed = s.target_speed;
    if (lookahead) *lookahead = s.lookahead;
    if (steer_gain) *steer_gain = s.steer_gain;
    if (epsilon) *epsilon = d->epsilon[slot];
    return CRL_OK;
}

int crl_car_driver_set_assignment(crl_car_driver *d, const int32_t *ids_dev, void *stream) {
    crl_fail_no_ctx();
    if (!d || !ids_dev) return crl_fail(CRL_EINVAL, "crl_car_driver_set_assignment: null argument");
    HIP_TRY(hipMemcpyAsync(d->assign, ids_dev, (size_t)d->n * d->players * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_car_driver_get_assignment(crl_car_driver *d, int32_t *ids_out_dev, void *stream) {
    crl_fail_no_ctx();
    if (!d || !ids_out_dev) return crl_fail(CRL_EINVAL, "crl_car_driver_get_assignment: null argument");
    HIP_TRY(hipMemcpyAsync(ids_out_dev, d->assign, (size_t)d->n * d->players * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CRL_OK;
}

int crl_car_driver_act(crl_car_driver *d, float *actions_dev, void *stream) {
    crl_fail_no_ctx();
    if (!d || !actions_dev) return crl_fail(CRL_EINVAL, "crl_car_driver_act: null argument");
    const CarSoA *s = crl_car_soa(d->car);
    DriverArgs A;
    A.body = s->body, A.done = s->done, A.ntiles = s->ntiles, A.tile_aabb_em = s->tile_aabb_em, A.assign = d->assign;
    A.n = d->n, A.players = d->players, A.call = d->calls, A.seed = d->seed, A.id_base = d->id_base;
    for (int k = 0; k < CRL_CAR_DRIVER_SLOTS; k++) A.style[k] = d->style[k];
    const unsigned blocks = (unsigned)((d->n + kDriverWaves - 1) / kDriverWaves);
    hipLaunchKernelGGL(car_driver_kernel, dim3(blocks), dim3(64 * kDriverWaves), 0, (hipStream_t)stream, A, actions_dev);
    HIP_TRY(hipGetLastError());
    d->calls++;
    return CRL_OK;
}

int crl_car_driver_get_counters(crl_car_driver *d, uint64_t *seed, int64_t *calls) {
    crl_fail_no_ctx();
    if (!d) return crl_fail(CRL_EINVAL, "crl_car_driver_get_counters: null driver");
    if (seed) *seed = d->seed;
    if (calls) *calls = (int64_t)d->calls;
    return CRL_OK;
}

int crl_car_driver_set_counters(crl_car_driver *d, uint64_t seed, int64_t calls) {
    crl_fail_no_ctx();
    if (calls < 0 || calls > 0xFFFFFFFFll) return crl_fail(CRL_EINVAL, "crl_car_driver_set_counters: calls must lie in [0, 2^32), not %lld", (long long)calls);
    if (!d) return crl_fail(CRL_EINVAL, "crl_car_driver_set_counters: null driver");
    d->seed = seed, d->calls = (uint32_t)calls;
    return CRL_OK;
}

}  // extern "C"

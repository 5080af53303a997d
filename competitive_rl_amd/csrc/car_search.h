// car_search.h -- what the servers beside a CarRacing context share (car_driver.hip, car_policy.hip): the generator of their draws,
// the wave's 64-bit minimum and the nearest-tile search of include/crl.h "car drivers" rule 2 for both cars of an env in one pass.
#pragma once
#include <math.h>

#include "car_device.h"

#pragma clang fp contract(off)

namespace crl {

// the generator of "league draws" (pong_device.h, car_track.hip)
__device__ inline void driver_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

__device__ inline uint64_t wave_min_u64(uint64_t k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), m, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)k, m, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        k = o < k ? o : k;
    }
    return k;
}

// Rule 2 for two points at once: the 64 lanes walk the env's n <= 512 boxes ([512] float4 of tile_aabb_em: 16 bytes per lane, 1 KiB
// per load), each box read once for both points; every lane keeps the smallest (distance, index) per point as one 64-bit key -- the
// distance's bit pattern above the index: distances are >= +0 or +inf, so the keys order as the rule does, the lowest index among
// equals included -- and six butterfly steps give every lane the wave's minimum.  No LDS, no barrier.
__device__ __forceinline__ void car_nearest2(const float4 *__restrict__ boxes, int n, int lane, float cx0, float cy0, float cx1, float cy1,
                                             int &near0, int &near1) {
    uint64_t best0 = ~0ull, best1 = ~0ull;
    for (int t = lane; t < n; t += 64) {
        const float4 b = boxes[t];
        const float tx = (b.x + b.z) * 0.5f, ty = (b.y + b.w) * 0.5f;
        const float dx0 = tx - cx0, dy0 = ty - cy0, dx1 = tx - cx1, dy1 = ty - cy1;
        float d0 = dx0 * dx0 + dy0 * dy0, d1 = dx1 * dx1 + dy1 * dy1;
        if (!(d0 == d0)) d0 = INFINITY;
        if (!(d1 == d1)) d1 = INFINITY;
        const uint64_t k0 = ((uint64_t)__float_as_uint(d0) << 32) | (uint32_t)t, k1 = ((uint64_t)__float_as_uint(d1) << 32) | (uint32_t)t;
        best0 = k0 < best0 ? k0 : best0;
        best1 = k1 < best1 ? k1 : best1;
    }
    near0 = (int)(uint32_t)wave_min_u64(best0), near1 = (int)(uint32_t)wave_min_u64(best1);
    near0 = (near0 >= 0 && near0 < n) ? near0 : 0;
    near1 = (near1 >= 0 && near1 < n) ? near1 : 0;
}

}  // namespace crl

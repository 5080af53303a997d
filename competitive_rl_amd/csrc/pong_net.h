// pong_net.h -- what the two served networks (pong_policy.hip, pong_policy_full.hip) share on the device: the vector types of the
// matrix instructions and conv1's exact bf16 operands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crl {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// conv1 on v_mfma_f32_16x16x32_bf16 at fp32 accuracy: the inputs are bytes -- exact in bf16 -- and a weight (pre-divided by 255) is
// the sum of three bf16 terms (8 + 8 + 8 mantissa bits), so the three products per tap are exact and accumulate in fp32.
__device__ inline void split_bf16x3(float w, __bf16 &h1, __bf16 &h2, __bf16 &h3) {
    h1 = (__bf16)w;
    const float r1 = w - (float)h1;  // exact
    h2 = (__bf16)r1;
    const float r2 = r1 - (float)h2;  // exact
    h3 = (__bf16)r2;
}

__device__ inline uint32_t pk_bytes_bf16(uint32_t two) {  // the two low bytes of `two` as a pair of bf16
    const bf2 v = {(__bf16)(float)(two & 255u), (__bf16)(float)((two >> 8) & 255u)};
    return __builtin_bit_cast(uint32_t, v);
}

}  // namespace crl

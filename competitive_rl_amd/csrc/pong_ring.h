// pong_ring.h -- the frame ring of the served Pong agents: the last four 42 x 42 opponent-view frames of every env, as
// pong_policy.hip, pong_policy_full.hip and pong_league.hip read and write it.  Plane j of the model's stack (oldest first) is ring
// plane (head + j) & 3: a new frame overwrites plane `head`, the oldest, in place, and `head` moves on by one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crl_internal.h"

namespace crl {

static constexpr int kDim = CRL_POLICY_DIM;                      // 42
static constexpr int kPlane = kDim * kDim;                       // 1764 bytes
static constexpr int kPlaneWords = kPlane / 4;                   // 441
static constexpr int kPlanePad = 1776;                           // a plane in the ring / in LDS: 111 16-byte chunks (12 bytes of padding)
static constexpr int kPlaneChunks = kPlanePad / 16;              // 111
static constexpr int kRingBytes = CRL_POLICY_STACK * kPlanePad;  // 7104 per env

// host: the frames and actions of an act call (`who`), as every kernel that pushes a frame into the ring needs them
inline int ring_check_act(const char *who, const uint8_t *frame_dev, int64_t frame_stride, int64_t action_stride) {
    if (frame_stride < kPlane || (frame_stride & 3) || ((uintptr_t)frame_dev & 3) || action_stride < 1)
        return crl_fail(CRL_EINVAL, "%s: frame_stride must be a multiple of 4 and >= 1764, frames 4-byte aligned", who);
    return CRL_OK;
}

inline hipError_t ring_reset(uint8_t *ring, int64_t n, hipStream_t st) { return hipMemsetAsync(ring, 0, (size_t)n * kRingBytes, st); }

// FrameStackTensor.update's mask (utils/utils.py:158-170) for a learner's ring: all four planes of every env whose byte in `reset`
// (u8 [n], device) is not 0 are zeroed, in front of the act launch that pushes the next frame (pong_policy.hip).  Each lane reads one
// flag, the wavefront ballots and zeroes the flagged envs' 7 104 bytes in 16-byte stores; one without a flag leaves after the ballot.
hipError_t ring_mask_reset(uint8_t *ring, const uint8_t *reset, int64_t n, hipStream_t st);

// ring <-> the model's stack (u8 [n][4][42][42], oldest first; tests, checkpoints): pong_policy.hip
hipError_t policy_copy_stack(uint8_t *ring, uint8_t *ext, int head, int64_t n, int to_ring, hipStream_t st);
// ... as the body of crl_*_get_stack / _set_stack (`who`) of an object T with a ring, its head and n
template <class T>
int ring_copy_stack(const char *who, T *o, const uint8_t *ext, int to_ring, void *stream) {
    crl_fail_no_ctx();
    if (!o || !ext) return crl_fail(CRL_EINVAL, "%s: null argument", who);
    HIP_TRY(policy_copy_stack(o->ring, const_cast<uint8_t *>(ext), o->head, o->n, to_ring, (hipStream_t)stream));
    return CRL_OK;
}

}  // namespace crl

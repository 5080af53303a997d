// pong_league.h -- what pong_league.hip (per-env opponents) uses of pong_policy.hip: the LightActorCritic kernel launched on an
// env-index list, and the ring <-> stack copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crl {

struct SampleArgs;  // pong_sample.h

static constexpr int kLightRawFloats = 1024 + 16 + 1024 + 16 + 4800 + 4;  // w1 | b1 | w2 | b2 | wa | ba (+ 1 pad), torch layouts

// once per process, before the first list launch (dynamic LDS size of the kernel)
hipError_t policy_light_list_prepare();
// One persistent launch for the envs env_list[0 .. *count_dev): ring planes, frames, actions and logits are addressed through the
// list.  `raw`: device floats in the layout above; `max_envs`: an upper bound of the count (sizes the grid); the list is 256-byte
// aligned and allocated in whole groups of 8 entries; `ticket`: a zeroed counter of this launch's own; `sample`: null = argmax, else
// include/crl.h "sampled actions" with these parameters (id_base: the global id of env 0 of the arrays the list indexes).
hipError_t policy_light_act_list(const float *raw, uint8_t *ring, int head, const uint8_t *frame, int64_t frame_stride, int32_t *actions,
                                 int64_t action_stride, float *logits, const int32_t *env_list, const unsigned *count_dev, int64_t max_envs, int cus,
                                 unsigned *ticket, const SampleArgs *sample, hipStream_t st);
// plane j of the model's stack (u8 [n][4][42][42], oldest first) is ring plane (head + j) & 3
hipError_t policy_copy_stack(uint8_t *ring, uint8_t *ext, int head, int64_t n, int to_ring, hipStream_t st);

}  // namespace crl

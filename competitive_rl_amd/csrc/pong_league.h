// pong_league.h -- what pong_league.hip (per-env opponents) uses of pong_policy.hip: the LightActorCritic's weight layout and its
// kernel launched on an env-index list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace crl {

struct SampleArgs;  // pong_sample.h

// a LightActorCritic's checkpoint tensors in one array, torch layouts: conv1 [16][4][4][4] | b1 | conv2 [16][16][2][2] | b2 | actor [3][1600] | ba (+ 1 pad)
static constexpr int kLightW1 = 0, kLightB1 = kLightW1 + 1024, kLightW2 = kLightB1 + 16, kLightB2 = kLightW2 + 1024, kLightWa = kLightB2 + 16;
static constexpr int kLightBa = kLightWa + 4800, kLightRawFloats = kLightBa + 4;
inline void policy_light_pack(float *raw, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *actor_w,
                              const float *actor_b) {
    memcpy(raw + kLightW1, conv1_w, 1024 * sizeof(float)), memcpy(raw + kLightB1, conv1_b, 16 * sizeof(float));
    memcpy(raw + kLightW2, conv2_w, 1024 * sizeof(float)), memcpy(raw + kLightB2, conv2_b, 16 * sizeof(float));
    memcpy(raw + kLightWa, actor_w, 4800 * sizeof(float)), memcpy(raw + kLightBa, actor_b, 3 * sizeof(float));
}

// once per process, before the first launch (dynamic LDS size of every instantiation of the kernel that this build launches)
hipError_t policy_light_prepare();
// One persistent launch for the envs env_list[0 .. *count_dev): ring planes, frames, actions and logits are addressed through the
// list.  `raw`: device floats in the layout above; `max_envs`: an upper bound of the count (sizes the grid); the list is 256-byte
// aligned and allocated in whole groups of 8 entries; `ticket`: a zeroed counter of this launch's own; `sample`: null = argmax, else
// include/crl.h "sampled actions" with these parameters (id_base: the global id of env 0 of the arrays the list indexes).
hipError_t policy_light_act_list(const float *raw, uint8_t *ring, int head, const uint8_t *frame, int64_t frame_stride, int32_t *actions,
                                 int64_t action_stride, float *logits, const int32_t *env_list, const unsigned *count_dev, int64_t max_envs, int cus,
                                 unsigned *ticket, const SampleArgs *sample, hipStream_t st);

}  // namespace crl

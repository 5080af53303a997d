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

// a crl_policy's blob carries the critic head behind it (crl_policy_set_critic / _load_weights; a league's slots end at kLightRawFloats):
// critic [1][1600] | bc (+ 3 pad)
static constexpr int kLightWc = kLightRawFloats, kLightBc = kLightWc + 1600, kLightCriticFloats = 1600 + 4;
inline void policy_light_pack_critic(float *critic_part /* raw + kLightWc */, const float *critic_w, const float *critic_b) {
    memcpy(critic_part, critic_w, 1600 * sizeof(float)), critic_part[1600] = critic_b[0];
}

// Weight reloads (crl_policy_load_weights, crl_pool_load_*): the blob is packed into ONE pinned host buffer, kept and reused, and
// copied to the device on the caller's stream -- act calls enqueued before the copy use the old weights, calls after it the new
// ones, and nothing synchronises the device.  The event marks the copy's end: the next reload waits on it (on the host) before it
// overwrites the buffer.
struct WeightStage {
    float *host = nullptr;
    size_t floats = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
};
// the buffer, free to be written, with room for `floats`
inline hipError_t weight_stage_begin(WeightStage &s, size_t floats) {
    hipError_t e = hipSuccess;
    if (s.pending) e = hipEventSynchronize(s.ev), s.pending = false;
    if (e == hipSuccess && !s.ev) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
    if (e == hipSuccess && s.floats < floats) {
        if (s.host) (void)hipHostFree(s.host), s.host = nullptr, s.floats = 0;
        e = hipHostMalloc((void **)&s.host, floats * sizeof(float), hipHostMallocDefault);
        if (e == hipSuccess) s.floats = floats;
    }
    return e;
}
// the first `floats` of the buffer -> dev, ordered on `st`
inline hipError_t weight_stage_send(WeightStage &s, float *dev, size_t floats, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(dev, s.host, floats * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(s.ev, st);
    if (e == hipSuccess) s.pending = true;
    return e;
}
inline void weight_stage_free(WeightStage &s) {
    if (s.pending) (void)hipEventSynchronize(s.ev);
    if (s.ev) (void)hipEventDestroy(s.ev);
    if (s.host) (void)hipHostFree(s.host);
    s = WeightStage{};
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

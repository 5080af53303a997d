// pong_policy_full.h -- the full-size ActorCritic (pong_policy_full.hip) as seen from pong_policy.hip and pong_league.hip, and the
// network's shapes and weight blob layout, which its learner (pong_ppo_full.hip) shares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crl {

static constexpr int kC1 = 16, kP1 = 400;  // conv1: 16 channels x 20 x 20
static constexpr int kC2 = 32, kP2 = 121;  // conv2: 32 channels x 11 x 11
static constexpr int kK3 = kC2 * kP2;      // 3872 = conv3's receptive field: the whole of act2
static constexpr int kC3 = 256;
// the packed blob, torch layouts: w1 | b1 | w2 | b2 | w3 | b3 | wa | ba + 1 pad (policy_full_pack), and behind it a crl_policy's and a
// learner's critic tail: wc | bc + 3 pad (policy_full_pack_critic)
static constexpr int kOffW1 = 0, kOffB1 = kOffW1 + 1024, kOffW2 = kOffB1 + 16, kOffB2 = kOffW2 + kC2 * 256, kOffW3 = kOffB2 + 32;
static constexpr int kOffB3 = kOffW3 + kC3 * kK3, kOffWa = kOffB3 + kC3, kOffBa = kOffWa + 3 * kC3, kFullRawFloats = kOffBa + 4;
static constexpr int kOffWc = kFullRawFloats, kOffBc = kOffWc + kC3, kFullCriticFloats = kC3 + 4;
static constexpr int kFullBlob = kFullRawFloats + kFullCriticFloats;  // 1 001 784

struct SampleArgs;  // pong_sample.h
struct HeadArgs;    // pong_sample.h

struct PolicyFull;  // device weights + activation scratch of one crl_policy

// weights: host pointers, torch layouts (conv1 [16][4][4][4], conv2 [32][16][4][4], conv3 [256][32][11][11], actor [3][256])
hipError_t policy_full_create(PolicyFull **out, int64_t num_envs, const float *conv1_w, const float *conv1_b, const float *conv2_w,
                              const float *conv2_b, const float *conv3_w, const float *conv3_b, const float *actor_w,
                              const float *actor_b);
void policy_full_destroy(PolicyFull *f);
// ring: the policy's frame ring (pong_ring.h), head: the plane to overwrite;
// sample: null = argmax, else include/crl.h "sampled actions" with these parameters
hipError_t policy_full_act(PolicyFull *f, uint8_t *ring, int head, int64_t n, const uint8_t *frame_dev, int64_t frame_stride,
                           int32_t *actions_dev, int64_t action_stride, float *logits_dev, const SampleArgs *sample, hipStream_t st);
// ... with the rollout heads (include/crl.h "rollout heads"): `values` / `logp`, float32 [n] on the device, each optional
hipError_t policy_full_act_heads(PolicyFull *f, uint8_t *ring, int head, int64_t n, const uint8_t *frame_dev, int64_t frame_stride,
                                 int32_t *actions_dev, int64_t action_stride, float *logits_dev, const SampleArgs *sample, float *values,
                                 float *logp, hipStream_t st);
// A crl_policy's blob carries the critic head (critic [1][256] | bc + 3 pad) behind policy_full_pack's: its device copy, the floats of
// the actor part (policy_full_blob_floats) and of the critic part, and the packing of the latter into critic_part[critic_floats].
float *policy_full_blob(PolicyFull *f);
int64_t policy_full_critic_floats();
void policy_full_pack_critic(float *critic_part, const float *critic_w, const float *critic_b);


// ---- the list form: a league's full-size agents (pong_league.hip).  The league owns the weight blobs and ONE activation scratch.
int64_t policy_full_blob_floats();  // floats of a packed weight blob (w1 | b1 | w2 | b2 | w3 | b3 | wa | ba)
int64_t policy_full_act2_floats();  // scratch floats per row: act2 [rows][3872] ...
int64_t policy_full_feat_floats();  // ... and feat [rows][256]
// host: packs the eight tensors (torch layouts, as policy_full_create takes them) into blob[policy_full_blob_floats()]
void policy_full_pack(float *blob, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *conv3_w,
                      const float *conv3_b, const float *actor_w, const float *actor_b);
// The three kernels for the envs env_list[0 .. *count_dev): row r of the compact scratch (act2 [scratch_rows][3872], feat
// [scratch_rows][256]) belongs to env env_list[r]; ring planes, frames, actions and logits are addressed through the list, and the
// frame of each listed env is pushed into its ring plane `head`.  The count is known on the device only: ceil(max_envs /
// scratch_rows) passes are launched, pass p serves list positions [p * scratch_rows, min(count, (p + 1) * scratch_rows)), a pass
// past the count is three launches that return at once.  Grids are persistent and sized from max_envs (an upper bound of the
// count) and `cus`.  `w_blob`: a device copy of policy_full_pack's blob; `sample`: null = argmax, else include/crl.h "sampled
// actions" with these parameters, drawn with the ENV's id (id_base: the global id of env 0 of the arrays the list indexes).
hipError_t policy_full_act_list(const float *w_blob, float *act2, float *feat, int64_t scratch_rows, uint8_t *ring, int head, const uint8_t *frame,
                                int64_t frame_stride, int32_t *actions, int64_t action_stride, float *logits, const int32_t *env_list,
                                const unsigned *count_dev, int64_t max_envs, int cus, const SampleArgs *sample, hipStream_t st);

}  // namespace crl

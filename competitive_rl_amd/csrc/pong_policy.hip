// pong_policy.hip -- the built-in CNN opponents of cPongTournament-v0 (WEAK / MEDIUM) on device.
//
// Restates Policy.__call__ (reference utils/policy_serving.py:46-66) with use_light_model=True:
// the policy keeps its own stack of the last four 42x42 frames it was shown
// (FrameStackTensor.update without a mask, utils/utils.py:159-170), runs LightActorCritic
// (utils/network.py:73-93) on it and plays the argmax of the three logits.
//
// One kernel per call: u8 frames in, int32 actions out; nothing else touches HBM but the 7 KB stack per env (pong_ring.h).  The two
// convolutions fuse exactly because conv2 is 2x2 with stride 2: each of the 10x10 conv2 positions owns its 2x2 block of conv1
// outputs (16 channels) and its 6x6x4 input patch.  516 800 FMAs per env in fp32 -- the reference is fp32, and bf16 / fp8
// activations would change which action wins in close calls -- on the matrix pipe (pong_policy_mfma_kernel below).  DESIGN.md 4c has
// the history; the packed-FMA kernel of round 1 is pong_policy_packed.inc, in the profiling build (-DCRL_ABLATION) only.
// The stack is a ring of four planes (padded to 111 16-byte chunks): the new frame overwrites the oldest plane in place, so a
// call reads 3 planes + the frame and writes 1 plane per env instead of rolling the stack; both go global -> LDS by LDS-DMA.
#include <stdlib.h>

#include <vector>

#include "crl_internal.h"
#include "pong_league.h"
#include "pong_net.h"
#include "pong_policy_full.h"
#include "pong_ring.h"
#include "pong_sample.h"

namespace crl {

static constexpr int kPos = 100;                       // 10 x 10 conv2 positions

// Request a group's data straight into LDS (global_load_lds: no registers are held while the loads are in flight):
// the three ring planes that stay (16-byte chunks, planes are padded to 111 chunks for this) and the new frame
// (dwords: frames are only 4-byte aligned) into the plane it replaces.  One wavefront-instruction fills a
// contiguous run of LDS (M0 = run base, lane l lands at base + l * size), so the work is cut into (env, plane,
// half) and (env, 64-dword run) pieces dealt to the eight wavefronts.
// Issued as inline asm: with the builtin the compiler assumes that any later LDS read may alias the transfer
// and waits for vmcnt(0) in front of the convolutions, which is exactly the overlap this is for.  The kernel
// waits itself (vmcnt(0) + barrier before the buffer is read).  M0 = LDS base of the run (one wait state
// between writing M0 and the LDS-DMA instruction); the compiler reserves M0 and sets it itself right before any
// instruction of its own that reads it.
typedef __attribute__((address_space(3))) void *lptr_t;
__device__ inline uint32_t lds_addr(const void *p) { return (uint32_t)(uintptr_t)(lptr_t)p; }
__device__ inline void lds_dma_b128(const void *src, uint32_t lds_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base)) : "memory");
}
__device__ inline void lds_dma_b32(const void *src, uint32_t lds_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base)) : "memory");
}

// ---------------------------------------------------------------------------------------------------------------
// The LightActorCritic on the matrix pipe (profiling build: CRL_POLICY_MFMA=0 selects the packed-FMA kernel of round 1 for A/B).
//
// v_mfma_f32_16x16x4_f32 multiplies exact f32 products at the vector peak (64 FLOP/clk/SIMD, MI355X_MICROARCH.md) but
// on the matrix pipe: the VALU stays free for the patch conversion, and the weights sit in VGPRs once per wavefront --
// no scalar weight stream, whose s_waitcnt in front of every 16 FMAs cost the packed-FMA kernel a third of its time.
//
// Both convolutions are computed TRANSPOSED, D^T[oc][pos] = W[oc][tap] x im2col^T[tap][pos], on tiles of 16 conv2
// positions q = env * 100 + pos2 (8 envs per group = 50 tiles, no padding):
//   conv1: the 2x2 conv1 outputs under a conv2 position form four parity CLASSES c = (ky0, kx0); per class one
//          accumulator tile D1[c] (rows = 16 output channels, cols = the 16 positions), 16 MFMAs each: step (ky, kx)
//          takes A = W1[oc = l & 15][ic = l >> 4][ky][kx] and B = x[ic = l >> 4][4 y2 + 2 ky0 + ky][4 x2 + 2 kx0 + kx] / 255
//          -- lane (position l & 15, plane l >> 4) needs the 6 x 6 patch of ONE plane: six aligned ds_read2_b32 per tile;
//   conv2: the accumulator layout (lane = position, registers r = channels 4 (l >> 4) + r) IS the B operand of the
//          next product: step (c, r) takes B = relu(D1[c][r]) as it stands and A = W2[oc2 = l & 15][ic = 4 (l >> 4) + r][c]
//          -- no transpose, no LDS round trip between the layers;
//   actor: each lane folds its four conv2 channels into three partial logits, two cross-lane adds finish the
//          position, and the 100 positions of an env are summed in a fixed shape (4 x 25, then 4) as before.
// 80 MFMAs per 16 positions = 500 per env: 65 536 envs x 500 x 32 cycles / 1 024 SIMDs = 1.02 M cycles (427 us at 2.4 GHz).
// One persistent 512-thread workgroup per CU -- two wavefronts per SIMD: a lone wavefront issues a vector instruction
// every 4 cycles, and the ~300 non-matrix instructions of a tile (gather, x / 255, relu, actor) next to its 80 MFMAs made
// the one-wavefront version 2.4x slower than the matrix pipe allows (1 018 us); with a partner, one's vector work runs
// under the other's MFMAs.  Groups are handed out by the ticket counter, the NEXT group's rings and frames land in the
// other half of a double buffer by LDS-DMA while this one is computed.
#ifndef CRL_MFMA_WAVES
#define CRL_MFMA_WAVES 8
#endif
#ifndef CRL_MFMA_PREFETCH
#define CRL_MFMA_PREFETCH 0
#endif
static constexpr int kME = 8;                       // envs per group
static constexpr int kMTiles = kME * kPos / 16;     // 50 tiles of 16 conv2 positions
static constexpr int kMWaves = CRL_MFMA_WAVES;                    // wavefronts per workgroup: two per SIMD (one gathers / converts while the other's MFMAs run)
static constexpr int kMThreads = 64 * kMWaves;
static constexpr int kMBuf = kME * CRL_POLICY_STACK * kPlanePad;  // 56 832 bytes per staging buffer
static constexpr int kMLdsRest = (3 * 1600 + 2 * kME * kPos * 3 + 4) * 4;
static constexpr int kMLds = 2 * kMBuf + kMLdsRest;
// VALUE instantiations: the critic is a fourth row of sh_wa.  A fourth column of sh_part beside it would need 164 880 bytes, 1 040 over
// the CU's 160 KiB, so the value's partials are reduced further inside the wavefront before they go to LDS: over the four positions
// 4 b .. 4 b + 3 of a BLOCK b.  Tiles (16 positions) and envs (100) both start at multiples of 4, so a block never straddles either
// and is the same four positions of the same env wherever the env sits in its group -- which a reduction over the whole tile,
// cut by the env's boundary, would not be.  25 floats per env instead of 100: 160 080 bytes in all.
static constexpr int kVBlocks = kPos / 4;  // 25 blocks per env
static constexpr int kMLdsValue = kMLds + (1600 + 2 * kME * kVBlocks) * 4;
static_assert(kMLdsValue <= 160 * 1024, "the VALUE instantiations' LDS must fit a CU");

// LIST: the group's eight envs are entries of an env-index list (the league, pong_league.hip) instead of env0 .. env0 + 7.  The
// entries sit in SGPRs before the first request of the group is issued (GroupIdx::load / pin): a load that returned between two
// LDS-DMA requests would be waited for with a vmcnt that drains the requests in front of it.
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
struct GroupIdx {
    i32x4 lo, hi;  // (two register vectors, constant subscripts only: nothing of this may live in scratch, whose loads count in vmcnt)
};
__device__ inline void group_idx_load(i32x4 &a, i32x4 &b, const int32_t *__restrict__ list, int64_t slot0) {
    const i32x4 *p = reinterpret_cast<const i32x4 *>(list + slot0);  // slot0 is a multiple of 8, the list 256-byte aligned and padded to whole groups
    a = p[0], b = p[1];
}
__device__ inline void group_idx_pin(GroupIdx &ix, i32x4 a, i32x4 b) {
    asm volatile("" : "+v"(a), "+v"(b));  // both loads have RETURNED here, in front of every later volatile statement (the requests)
    ix.lo = i32x4{__builtin_amdgcn_readfirstlane(a.x), __builtin_amdgcn_readfirstlane(a.y), __builtin_amdgcn_readfirstlane(a.z), __builtin_amdgcn_readfirstlane(a.w)};
    ix.hi = i32x4{__builtin_amdgcn_readfirstlane(b.x), __builtin_amdgcn_readfirstlane(b.y), __builtin_amdgcn_readfirstlane(b.z), __builtin_amdgcn_readfirstlane(b.w)};
}
template <bool LIST>
__device__ inline int64_t group_env(const GroupIdx ix, int64_t env0, int fe) {
    if constexpr (!LIST) return env0 + fe;
    int32_t e = ix.lo.x;
    e = fe == 1 ? ix.lo.y : e, e = fe == 2 ? ix.lo.z : e, e = fe == 3 ? ix.lo.w : e;
    e = fe == 4 ? ix.hi.x : e, e = fe == 5 ? ix.hi.y : e, e = fe == 6 ? ix.hi.z : e, e = fe == 7 ? ix.hi.w : e;
    return e;
}

template <bool LIST>
__device__ inline void group_request_m(uint8_t *shbuf, const uint8_t *__restrict__ ring, int head, const uint8_t *__restrict__ frame,
                                       int64_t frame_stride, int64_t env0, const GroupIdx ix, int envs_here, int wave, int lane) {
    for (int s = wave; s < kME * 3; s += kMWaves) {
        const int fe = s / 3, j = s - fe * 3;
        if (fe >= envs_here) continue;
        const int pp = (head + 1 + j) & 3;
        const uint8_t *src = ring + group_env<LIST>(ix, env0, fe) * (int64_t)kRingBytes + pp * kPlanePad;
        uint8_t *dst = shbuf + (fe * CRL_POLICY_STACK + pp) * kPlanePad;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int c = half * 64 + lane;
            if (c < kPlaneChunks) lds_dma_b128(src + c * 16, lds_addr(dst + half * 1024));
        }
    }
    for (int s = wave; s < kME * 7; s += kMWaves) {
        const int fe = s / 7, q = s - fe * 7;
        if (fe >= envs_here) continue;
        const int d = q * 64 + lane;
        const uint8_t *src = frame + group_env<LIST>(ix, env0, fe) * frame_stride;
        uint8_t *dst = shbuf + (fe * CRL_POLICY_STACK + head) * kPlanePad + q * 256;
        if (d < kPlaneWords) lds_dma_b32(src + d * 4, lds_addr(dst));
    }
}

struct PolicyWeightsM {
    const float *w1, *b1, *w2, *b2, *wa, *ba;  // torch layouts: conv1 [16][4][4][4], conv2 [16][16][2][2], actor [3][1600]
};

// BF = true: conv1 on the bf16 matrix instruction at fp32 accuracy (pong_net.h: bytes and three-term weights, all products
// exact): 6 instructions x 16 cycles per parity class instead of 16 x 32, and the patch conversion shrinks from 36 correctly
// rounded x / 255 to 48 byte -> bf16 conversions.
// LIST: env_list[0 .. *count_dev) are the envs of this launch (`n_arg` is unused; the host does not know the count after a device-side
// re-draw, so the grid is sized by an upper bound and a launch with an empty list ends at once); every ring, frame, action and logit
// address goes through the list.  An env's logits are reduced in a shape of their own (finish_group), so its action does not depend
// on which group or slot it sits in.  LIST = false is the launch of crl_policy_act.
// SAMPLE: the lane that writes an env's action draws it by include/crl.h "sampled actions" (sample_action, one Philox call) instead of
// keeping the argmax.  A template parameter, not a branch on a kernel argument: the greedy instantiations are then the code they were
// (same registers, same LDS, same schedule around the matrix instructions), whatever the compiler makes of the sampling epilogue.
// VALUE (crl_policy_act_rollout with values or log-probs; dense only): the critic head beside the actor -- a fourth partial per lane over
// the same four channels, fmaf by fmaf, summed in a fixed shape of its own (four positions in the wavefront, then 25 blocks in
// finish_group) -- and the epilogue's value / log-prob stores (H).  A template parameter like SAMPLE, for the same reason.
template <bool BF, bool LIST, bool SAMPLE, bool VALUE = false>
__global__ __launch_bounds__(kMThreads, 1) void pong_policy_mfma_kernel(PolicyWeightsM W, uint8_t *__restrict__ ring, int head,
                                                                  const uint8_t *__restrict__ frame, int64_t frame_stride,
                                                                  int32_t *__restrict__ actions, int64_t action_stride,
                                                                  float *__restrict__ logits_out, int64_t n_arg, unsigned *__restrict__ ticket,
                                                                  const int32_t *__restrict__ env_list, const unsigned *__restrict__ count_dev, SampleArgs S, HeadArgs H) {
    const int64_t n = LIST ? (int64_t)*count_dev : n_arg;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *sh_buf = smem;                                             // [2][kME][4][kPlanePad]
    float *sh_wa = reinterpret_cast<float *>(smem + 2 * kMBuf);         // [3][1600]; VALUE: [4][1600], the critic last
    float *sh_part = sh_wa + (VALUE ? 4 : 3) * 1600;                    // [2][kME * 100][3]: a group's partial logits, double-buffered
    float *sh_vpart = sh_part + 2 * kME * kPos * 3;                     // VALUE: [2][kME * 25]: its partial values, one per block of four positions
    unsigned *sh_ticket = reinterpret_cast<unsigned *>(sh_vpart + (VALUE ? 2 * kME * kVBlocks : 0));  // [2]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lj = lane & 15, lk = lane >> 4;
    const int64_t ngroups = (n + kME - 1) / kME;

    for (int i = tid; i < 3 * 1600; i += kMThreads) sh_wa[i] = W.wa[i];
    if constexpr (VALUE)
        for (int i = tid; i < 1600; i += kMThreads) sh_wa[3 * 1600 + i] = H.wc[i];
    // the wavefront's weights, once: A operands of every MFMA step
    float w1[16], w2[4][4];
    bf8 wA[3][2];  // BF: A[oc = lj][k = 32 i + 8 lk + j], k = ic * 16 + ky * 4 + kx (torch's own order), as three bf16 terms
    if constexpr (BF) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                __bf16 h1, h2, h3;
                split_bf16x3(W.w1[lj * 64 + 32 * i + 8 * lk + j] / 255.0f, h1, h2, h3);
                wA[0][i][j] = h1, wA[1][i][j] = h2, wA[2][i][j] = h3;
            }
#pragma unroll
        for (int s = 0; s < 16; s++) w1[s] = 0.f;
    } else {
#pragma unroll
        for (int s = 0; s < 16; s++) w1[s] = W.w1[lj * 64 + lk * 16 + s];                  // W1[oc = lj][ic = lk][ky = s / 4][kx = s % 4]
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) w2[c][r] = W.w2[(lj * 16 + 4 * lk + r) * 4 + c];      // W2[oc2 = lj][ic = 4 lk + r][ky0, kx0 = c]
    f4 bias1, bias2;
#pragma unroll
    for (int r = 0; r < 4; r++) bias1[r] = W.b1[4 * lk + r], bias2[r] = W.b2[4 * lk + r];  // D rows = channels 4 lk + r
    float ba0 = W.ba[0], ba1 = W.ba[1], ba2 = W.ba[2];
    float bc = 0.f;
    if constexpr (VALUE) bc = H.bc[0];
    // Every load above must have RETURNED before the first LDS-DMA request is issued: the compiler waits for a load at its
    // first use with a vmcnt(N) that counts only the loads it knows of -- inside the tile loop that wait would also drain
    // the next group's LDS-DMA transfers (inline asm, invisible to it) and serialise staging with the convolutions.
    if constexpr (BF) {
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int i = 0; i < 2; i++) {
                u32x4 bits = __builtin_bit_cast(u32x4, wA[t][i]);
                asm volatile("" : "+v"(bits));
                wA[t][i] = __builtin_bit_cast(bf8, bits);
            }
    } else {
#pragma unroll
        for (int s = 0; s < 16; s++) asm volatile("" : "+v"(w1[s]));
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) asm volatile("" : "+v"(w2[c][r]));
    asm volatile("" : "+v"(bias1), "+v"(bias2), "+v"(ba0), "+v"(ba1), "+v"(ba2));
    if constexpr (VALUE) asm volatile("" : "+v"(bc));
    __syncthreads();  // sh_wa is staged

    // Three groups are in play: g (being computed), g1 (streaming into the other buffer) and the ticket for the one after
    // (a returning global atomic takes microseconds: it is requested at the top of an iteration and read at its end).
    int64_t g = blockIdx.x, g1 = ngroups, gprev = -1;
    int cur = 0;  // parity of the group being computed: staging buffer, partial buffer; the ticket lands in slot cur ^ 1
    const i32x4 zero4 = {0, 0, 0, 0};
    GroupIdx ix_prev = {zero4, zero4}, ix_cur = ix_prev, ix_next = ix_prev;  // LIST: the list entries of groups gprev, g, g1
    if (g < ngroups) {
        const int64_t env0 = g * kME;
        if (tid == 0) sh_ticket[0] = atomicAdd(ticket, 1u);
        if constexpr (LIST) {
            i32x4 ia, ib;
            group_idx_load(ia, ib, env_list, env0);
            group_idx_pin(ix_cur, ia, ib);
        }
        group_request_m<LIST>(sh_buf, ring, head, frame, frame_stride, env0, ix_cur, (int)((n - env0) < kME ? (n - env0) : kME), wave, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        g1 = (int64_t)gridDim.x + sh_ticket[0];
    }
    // A finished group's 100 partial logits per env and action are summed in a fixed shape (lane j: positions j, j + 32, j + 64,
    // j + 96; then a 32-lane butterfly) by ONE wavefront per env, at the top of the NEXT group's iteration -- beside the other
    // wavefronts' matrix work instead of between two workgroup barriers.
    auto finish_group = [&](int64_t gp, int par, const GroupIdx ixg) {
        const int64_t e0 = gp * kME;
        const int envs = (int)((n - e0) < kME ? (n - e0) : kME);
        const float *part = sh_part + par * (kME * kPos * 3);
        for (int pe = wave; pe < envs; pe += kMWaves) {
            const int j = lane & 31;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int pos = j + 32 * m;
                if (pos < kPos) {
                    const float *pp = part + (pe * kPos + pos) * 3;
                    s0 += pp[0], s1 += pp[1], s2 += pp[2];
                }
            }
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) s0 += __shfl_xor(s0, d), s1 += __shfl_xor(s1, d), s2 += __shfl_xor(s2, d);
            if constexpr (VALUE) {  // the env's 25 block sums: lane j takes block j, the same 32-lane butterfly
                float sv = j < kVBlocks ? sh_vpart[par * (kME * kVBlocks) + pe * kVBlocks + j] : 0.f;
#pragma unroll
                for (int d = 16; d >= 1; d >>= 1) sv += __shfl_xor(sv, d);
                if (lane == 0)
                    action_epilogue<SAMPLE, true>(S, group_env<LIST>(ixg, e0, pe), ba0 + s0, ba1 + s1, ba2 + s2, actions, action_stride, logits_out, bc + sv, &H);
            } else {
                if (lane == 0) action_epilogue<SAMPLE>(S, group_env<LIST>(ixg, e0, pe), ba0 + s0, ba1 + s1, ba2 + s2, actions, action_stride, logits_out);
            }
        }
    };
    while (g < ngroups) {
        const int64_t env0 = g * kME;
        const int envs_here = (int)((n - env0) < kME ? (n - env0) : kME);
        uint8_t *buf = sh_buf + cur * kMBuf;
        float *part_out = sh_part + cur * (kME * kPos * 3);
        if (tid == 0) sh_ticket[cur ^ 1] = atomicAdd(ticket, 1u);
        // LIST: the next group's list entries are requested here and awaited behind the reduction and the write-back below -- the
        // one place of the iteration where nothing of this workgroup is in flight that the wait could drain
        i32x4 ia, ib;
        if constexpr (LIST)
            if (g1 < ngroups) group_idx_load(ia, ib, env_list, g1 * kME);
        if (gprev >= 0) finish_group(gprev, cur ^ 1, ix_prev);
        if constexpr (!LIST)
            if (g1 < ngroups) {  // the next group streams into the other buffer during the convolutions
                const int64_t e1 = g1 * kME;
                group_request_m<false>(sh_buf + (cur ^ 1) * kMBuf, ring, head, frame, frame_stride, e1, ix_next, (int)((n - e1) < kME ? (n - e1) : kME), wave, lane);
            }
        // the new frame also replaces plane `head` of the ring in HBM
        for (int i = tid; i < envs_here * kPlaneChunks; i += kMThreads) {
            const int fe = i / kPlaneChunks, c = i - fe * kPlaneChunks;
            reinterpret_cast<uint4 *>(ring + group_env<LIST>(ix_cur, env0, fe) * (int64_t)kRingBytes + head * kPlanePad)[c] =
                reinterpret_cast<const uint4 *>(buf + (fe * CRL_POLICY_STACK + head) * kPlanePad)[c];
        }
        if constexpr (LIST)
            if (g1 < ngroups) {
                const int64_t e1 = g1 * kME;
                group_idx_pin(ix_next, ia, ib);
                group_request_m<true>(sh_buf + (cur ^ 1) * kMBuf, ring, head, frame, frame_stride, e1, ix_next, (int)((n - e1) < kME ? (n - e1) : kME), wave, lane);
            }
        // The patch of tile t + kMWaves is gathered and converted WHILE tile t's MFMAs run: the two are independent, so the
        // scheduler threads the vector work between the matrix instructions (a wavefront that converts first and multiplies
        // afterwards leaves the matrix pipe idle 44 % of the time even with a partner on the SIMD).
        auto gather = [&](int t, float (&xo)[6][6]) {
            const int q = 16 * t + lj, e = q / kPos, pos = q - e * kPos, y2 = pos / 10, x2 = pos - y2 * 10;
            // this lane's 6 x 6 patch of plane ic = lk, as x / 255 (correctly rounded: Markstein).  Two ALIGNED dwords per 6-byte
            // row piece: (4 y2 + r) * 42 + 4 x2 is a multiple of 4 for even r and 2 past one for odd r -- known at compile time.
            const float rcp = 1.0f / 255.0f;
            const uint8_t *base = buf + (e * CRL_POLICY_STACK + ((head + 1 + lk) & 3)) * kPlanePad + (4 * y2) * kDim + 4 * x2;
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const uint32_t *p32 = reinterpret_cast<const uint32_t *>(base + r * kDim - 2 * (r & 1));
                uint32_t w0 = p32[0], w1_ = p32[1];
                if (r & 1) w0 = (w0 >> 16) | (w1_ << 16), w1_ >>= 16;
                const float b[6] = {(float)(w0 & 255u), (float)((w0 >> 8) & 255u), (float)((w0 >> 16) & 255u), (float)(w0 >> 24),
                                    (float)(w1_ & 255u), (float)((w1_ >> 8) & 255u)};
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const float qv = b[k] * rcp;
                    const float rem = __builtin_fmaf(qv, -255.0f, b[k]);
                    xo[r][k] = __builtin_fmaf(rem, rcp, qv);
                }
            }
        };
        // BF: lane (position lj, k-block lk) needs, of planes lk >> 1 and 2 + (lk >> 1), rows 4 y2 + 2 (lk & 1) + 0..3 and the six
        // columns from 4 x2 on: the B operand of (class (ky0, kx0), K half i) is rows 2 ky0, 2 ky0 + 1 of that window, columns
        // 2 kx0 .. 2 kx0 + 3, of plane 2 i + (lk >> 1) -- eight bf16 in k order.  Same aligned-dword trick as above.
        auto gather_bf = [&](int t, bf8 (&bx)[4][2]) {
            const int q = 16 * t + lj, e = q / kPos, pos = q - e * kPos, y2 = pos / 10, x2 = pos - y2 * 10;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int plane = 2 * i + (lk >> 1);
                const uint8_t *base = buf + (e * CRL_POLICY_STACK + ((head + 1 + plane) & 3)) * kPlanePad + (4 * y2 + 2 * (lk & 1)) * kDim + 4 * x2;
                uint32_t pk[4][3];  // per window row: columns (0,1) (2,3) (4,5) as bf16 pairs
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const uint32_t *p32 = reinterpret_cast<const uint32_t *>(base + rr * kDim - 2 * (rr & 1));
                    uint32_t w0 = p32[0], w1_ = p32[1];
                    if (rr & 1) w0 = (w0 >> 16) | (w1_ << 16), w1_ >>= 16;
                    pk[rr][0] = pk_bytes_bf16(w0), pk[rr][1] = pk_bytes_bf16(w0 >> 16), pk[rr][2] = pk_bytes_bf16(w1_);
                }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int ky0 = c >> 1, kx0 = c & 1;
                    const u32x4 v = {pk[2 * ky0][kx0], pk[2 * ky0][kx0 + 1], pk[2 * ky0 + 1][kx0], pk[2 * ky0 + 1][kx0 + 1]};
                    bx[c][i] = __builtin_bit_cast(bf8, v);
                }
            }
        };
        float xnext[6][6];
        if (CRL_MFMA_PREFETCH && !BF && wave < kMTiles) gather(wave, xnext);
        for (int t = wave; t < kMTiles; t += kMWaves) {
            const int q = 16 * t + lj, e = q / kPos, pos = q - e * kPos;
            float xin[6][6];
            bf8 bx[4][2];
            if constexpr (BF) {
                gather_bf(t, bx);
            } else if (CRL_MFMA_PREFETCH) {
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int k = 0; k < 6; k++) xin[r][k] = xnext[r][k];
                if (t + kMWaves < kMTiles) gather(t + kMWaves, xnext);
            } else {
                gather(t, xin);
            }
            // ---- conv1: four parity classes, 16 MFMAs each (independent accumulator chains)
            f4 d1[4] = {bias1, bias1, bias1, bias1};
            if constexpr (BF) {
#pragma unroll
                for (int tm = 2; tm >= 0; tm--)  // smallest weight term first
#pragma unroll
                    for (int i = 0; i < 2; i++)
#pragma unroll
                        for (int c = 0; c < 4; c++) d1[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wA[tm][i], bx[c][i], d1[c], 0, 0, 0);
            } else {
#pragma unroll
                for (int s = 0; s < 16; s++)
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        d1[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], xin[2 * (c >> 1) + (s >> 2)][2 * (c & 1) + (s & 3)], d1[c], 0, 0, 0);
            }
            // ---- conv2: the accumulators are the B operands as they stand
            f4 d2a = bias2, d2b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float hval = fmaxf(d1[c][r], 0.f);
                    if ((c * 4 + r) & 1) d2b = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[c][r], hval, d2b, 0, 0, 0);
                    else d2a = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[c][r], hval, d2a, 0, 0, 0);
                }
            // ---- actor: lane (position lj, channels 4 lk + r)
            float l0 = 0.f, l1 = 0.f, l2 = 0.f, lv = 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float f = fmaxf(d2a[r] + d2b[r], 0.f);
                const int wi = (4 * lk + r) * kPos + pos;
                l0 = __builtin_fmaf(sh_wa[wi], f, l0);
                l1 = __builtin_fmaf(sh_wa[1600 + wi], f, l1);
                l2 = __builtin_fmaf(sh_wa[3200 + wi], f, l2);
                if constexpr (VALUE) lv = __builtin_fmaf(sh_wa[4800 + wi], f, lv);
            }
            // the four channel groups of a position sit 16 lanes apart: (g0 + g1) + (g2 + g3), a fixed order
            l0 += __shfl_xor(l0, 16), l1 += __shfl_xor(l1, 16), l2 += __shfl_xor(l2, 16);
            l0 += __shfl_xor(l0, 32), l1 += __shfl_xor(l1, 32), l2 += __shfl_xor(l2, 32);
            if (lk == 0) part_out[q * 3 + 0] = l0, part_out[q * 3 + 1] = l1, part_out[q * 3 + 2] = l2;
            if constexpr (VALUE) {  // channel groups as above, then the block's four positions (lanes lj ^ 1, lj ^ 2): one float per block
                lv += __shfl_xor(lv, 16), lv += __shfl_xor(lv, 32);
                lv += __shfl_xor(lv, 1), lv += __shfl_xor(lv, 2);
                if (lk == 0 && (lj & 3) == 0) sh_vpart[cur * (kME * kVBlocks) + (q >> 2)] = lv;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's share of the next group has landed (and the ticket is back)
        __syncthreads();                                    // ... everybody's has, and every tile of this group is in part_out
        gprev = g;
        g = g1;
        g1 = (int64_t)gridDim.x + sh_ticket[cur ^ 1];
        cur ^= 1;
        if constexpr (LIST) ix_prev = ix_cur, ix_cur = ix_next;
    }
    if (gprev >= 0) finish_group(gprev, cur ^ 1, ix_prev);
}

// ring <-> logical order (tests, checkpoints): plane j of the model's stack is ring plane (head + j) & 3
__global__ void pong_policy_copy_stack_kernel(uint8_t *__restrict__ ring, uint8_t *__restrict__ ext, int head, int64_t words, int to_ring) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    const int64_t env = i / (CRL_POLICY_STACK * kPlaneWords);
    const int r = (int)(i - env * (CRL_POLICY_STACK * kPlaneWords));
    const int j = r / kPlaneWords, d = r - j * kPlaneWords;
    uint32_t *rp = reinterpret_cast<uint32_t *>(ring) + env * (kRingBytes / 4) + ((head + j) & 3) * (kPlanePad / 4) + d;
    uint32_t *ep = reinterpret_cast<uint32_t *>(ext) + i;
    if (to_ring) *rp = *ep;
    else *ep = *rp;
}

// pong_ring.h ring_mask_reset: a lane per env flag, a wavefront per flagged env's 444 16-byte chunks
__global__ __launch_bounds__(256) void pong_ring_mask_reset_kernel(uint8_t *__restrict__ ring, const uint8_t *__restrict__ reset, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long m = __ballot(i < n && reset[i] != 0);
    const int64_t w0 = i - lane;
    while (m) {  // (uniform; a wavefront without a flag leaves here)
        const int b = __ffsll(m) - 1;
        m &= m - 1;
        uint4 *dst = reinterpret_cast<uint4 *>(ring + (w0 + b) * (int64_t)kRingBytes);  // (w0 + b < n: the flag was read there)
#pragma unroll
        for (int q = 0; q < (kRingBytes / 16 + 63) / 64; q++) {
            const int c = q * 64 + lane;
            if (c < kRingBytes / 16) dst[c] = uint4{0u, 0u, 0u, 0u};
        }
    }
}

hipError_t ring_mask_reset(uint8_t *ring, const uint8_t *reset, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(pong_ring_mask_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ring, reset, n);
    return hipGetLastError();
}

hipError_t policy_copy_stack(uint8_t *ring, uint8_t *ext, int head, int64_t n, int to_ring, hipStream_t st) {
    const int64_t words = n * CRL_POLICY_STACK * kPlaneWords;
    hipLaunchKernelGGL(pong_policy_copy_stack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, ring, ext, head, words, to_ring);
    return hipGetLastError();
}

// ---- the launches of pong_policy_mfma_kernel: crl_policy_act below and the league's lists (pong_league.h)
static PolicyWeightsM light_weights(const float *raw) {  // raw: device floats, pong_league.h's layout
    return PolicyWeightsM{raw + kLightW1, raw + kLightB1, raw + kLightW2, raw + kLightB2, raw + kLightWa, raw + kLightBa};
}

// every instantiation this build launches, with its dynamic LDS: [list * 2 + sample], [4 + sample] the dense rollout launch (VALUE);
// profiling build: [6 + sample] is conv1 on the fp32 matrix instruction
typedef decltype(&pong_policy_mfma_kernel<true, false, false>) MfmaKernel;
struct MfmaEntry {
    MfmaKernel kernel;
    int lds;
};
static const MfmaEntry kMfmaKernels[] = {
    {pong_policy_mfma_kernel<true, false, false>, kMLds},            {pong_policy_mfma_kernel<true, false, true>, kMLds},
    {pong_policy_mfma_kernel<true, true, false>, kMLds},             {pong_policy_mfma_kernel<true, true, true>, kMLds},
    {pong_policy_mfma_kernel<true, false, false, true>, kMLdsValue}, {pong_policy_mfma_kernel<true, false, true, true>, kMLdsValue},
#ifdef CRL_ABLATION
    {pong_policy_mfma_kernel<false, false, false>, kMLds},           {pong_policy_mfma_kernel<false, false, true>, kMLds},
#endif
};

hipError_t policy_light_prepare() {
    hipError_t e = hipSuccess;
    for (const MfmaEntry &k : kMfmaKernels)
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k.lds);
    return e;
}

// One persistent launch, a workgroup per CU at the most.  env_list / count_dev: the LIST form (`n` is then an upper bound of the count,
// which the kernel reads itself), else null; sample: null = argmax; bf = false: profiling build only, dense only; heads: the rollout
// launch (dense, bf only), else null.
static hipError_t policy_mfma_launch(bool bf, const float *raw, uint8_t *ring, int head, const uint8_t *frame, int64_t frame_stride, int32_t *actions,
                                     int64_t action_stride, float *logits, int64_t n, int cus, unsigned *ticket, const int32_t *env_list,
                                     const unsigned *count_dev, const SampleArgs *sample, const HeadArgs *heads, hipStream_t st) {
    const int64_t groups = (n + kME - 1) / kME;
    const unsigned grid = (unsigned)(groups < cus ? groups : cus);
    const MfmaEntry &k = kMfmaKernels[(heads ? 4 : CRL_ABL(!bf) ? 6 : env_list ? 2 : 0) + (sample ? 1 : 0)];
    hipLaunchKernelGGL(k.kernel, dim3(grid), dim3(kMThreads), k.lds, st, light_weights(raw), ring, head, frame, frame_stride, actions, action_stride, logits,
                       env_list ? (int64_t)0 : n, ticket, env_list, count_dev, sample ? *sample : SampleArgs{}, heads ? *heads : HeadArgs{});
    return hipGetLastError();
}

hipError_t policy_light_act_list(const float *raw, uint8_t *ring, int head, const uint8_t *frame, int64_t frame_stride, int32_t *actions,
                                 int64_t action_stride, float *logits, const int32_t *env_list, const unsigned *count_dev, int64_t max_envs, int cus,
                                 unsigned *ticket, const SampleArgs *sample, hipStream_t st) {
    return policy_mfma_launch(true, raw, ring, head, frame, frame_stride, actions, action_stride, logits, max_envs, cus, ticket, env_list, count_dev,
                              sample, nullptr, st);
}

#ifdef CRL_ABLATION
#include "pong_policy_packed.inc"
#endif

}  // namespace crl

using namespace crl;

struct crl_policy {
    int device = 0;
    int64_t n = 0;
    int cus = 256;
    int head = 0;  // ring plane holding the OLDEST frame (the next one to be replaced)
    uint8_t *ring = nullptr;
    unsigned *ticket = nullptr;  // next group to hand out (reset before every launch)
    float *raw = nullptr;        // the checkpoint tensors in torch layout (pong_league.h kLightRawFloats)
    PolicyFull *full = nullptr;  // crl_policy_create_full: ActorCritic instead of LightActorCritic (pong_policy_full.hip)
    bool sampling = false;       // crl_policy_set_sampling with a temperature or an epsilon that is not 0: the SAMPLE kernels
    SampleArgs S{};              // S.n: crl_policy_act / _act_rollout calls since create / crl_policy_set_sampling
    float temperature = 0.f, epsilon = 0.f;  // ... as crl_policy_set_sampling took them (crl_policy_get_sampling)
    bool critic = false;         // crl_policy_set_critic / _load_weights gave a critic head (the blob's tail, zero until then)
    WeightStage stage{};         // crl_policy_load_weights: the pinned host copy of the blob
#ifdef CRL_ABLATION
    PolicyWeights packed{};      // the packed-FMA kernel's weight stream
#endif
};

extern "C" {

int crl_policy_create(int32_t device, int64_t num_envs, const float *conv1_w, const float *conv1_b, const float *conv2_w,
                      const float *conv2_b, const float *actor_w, const float *actor_b, crl_policy **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b)
        return crl_fail(CRL_EINVAL, "crl_policy_create: bad arguments");
    HIP_TRY(hipSetDevice(device));
    crl_policy *p = new crl_policy();
    p->device = device, p->n = num_envs;
    if (hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || p->cus <= 0) p->cus = 256;
    std::vector<float> raw(kLightRawFloats + kLightCriticFloats, 0.f);  // (the critic part stays zero until crl_policy_set_critic / _load_weights)
    policy_light_pack(raw.data(), conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b);
    hipError_t e = hipMalloc(&p->raw, raw.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(p->raw, raw.data(), raw.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->ticket, sizeof(unsigned));
    if (e == hipSuccess) e = hipMalloc(&p->ring, (size_t)num_envs * kRingBytes);
    if (e == hipSuccess) e = hipMemset(p->ring, 0, (size_t)num_envs * kRingBytes);
    if (e == hipSuccess) e = policy_light_prepare();
#ifdef CRL_ABLATION
    if (e == hipSuccess) e = packed_policy_create(p->packed, conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b);
#endif
    if (e != hipSuccess) {
        crl_policy_destroy(p);
        return crl_hip_fail(e, "crl_policy_create");
    }
    *out = p;
    return CRL_OK;
}

int crl_policy_create_full(int32_t device, int64_t num_envs, const float *conv1_w, const float *conv1_b, const float *conv2_w,
                           const float *conv2_b, const float *conv3_w, const float *conv3_b, const float *actor_w, const float *actor_b,
                           crl_policy **out) {
    crl_fail_no_ctx();
    if (!out || num_envs <= 0 || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !conv3_w || !conv3_b || !actor_w || !actor_b)
        return crl_fail(CRL_EINVAL, "crl_policy_create_full: bad arguments");
    HIP_TRY(hipSetDevice(device));
    crl_policy *p = new crl_policy();
    p->device = device, p->n = num_envs;
    hipError_t e = hipMalloc(&p->ring, (size_t)num_envs * kRingBytes);
    if (e == hipSuccess) e = hipMemset(p->ring, 0, (size_t)num_envs * kRingBytes);
    if (e == hipSuccess) e = policy_full_create(&p->full, num_envs, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, actor_w, actor_b);
    if (e != hipSuccess) {
        crl_policy_destroy(p);
        return crl_hip_fail(e, "crl_policy_create_full");
    }
    *out = p;
    return CRL_OK;
}

void crl_policy_destroy(crl_policy *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    weight_stage_free(p->stage);
    policy_full_destroy(p->full);
#ifdef CRL_ABLATION
    if (p->packed.stream) (void)hipFree(const_cast<float *>(p->packed.stream));
#endif
    if (p->raw) (void)hipFree(p->raw);
    if (p->ring) (void)hipFree(p->ring);
    if (p->ticket) (void)hipFree(p->ticket);
    delete p;
}

int crl_policy_reset(crl_policy *p, void *stream) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_policy_reset: null policy");
    HIP_TRY(ring_reset(p->ring, p->n, (hipStream_t)stream));
    p->head = 0;
    return CRL_OK;
}

// crl_policy_act (`who`; reset, values and logp null) and crl_policy_act_rollout.  Without values and log-probs the launches are
// crl_policy_act's own; with either, the VALUE instantiations / the full-size actor with the critic row.
static int policy_act(const char *who, crl_policy *p, const uint8_t *frame_dev, int64_t frame_stride, const uint8_t *reset_dev, int32_t *actions_dev,
                      int64_t action_stride, float *logits_dev, float *values_dev, float *logp_dev, void *stream) {
    crl_fail_no_ctx();
    if (!p || !frame_dev || !actions_dev) return crl_fail(CRL_EINVAL, "%s: null argument", who);
    if (int rc = ring_check_act(who, frame_dev, frame_stride, action_stride)) return rc;
    if (values_dev && !p->critic) return crl_fail(CRL_EINVAL, "%s: values_dev, but the policy has no critic (crl_policy_set_critic / _load_weights)", who);
    hipStream_t st = (hipStream_t)stream;
    if (reset_dev) HIP_TRY(ring_mask_reset(p->ring, reset_dev, p->n, st));
    const SampleArgs S = p->S;  // this call's counter; the next call's is one further, whichever kernel serves it
    p->S.n++;
    const SampleArgs *sample = p->sampling ? &S : nullptr;
    const bool heads = values_dev || logp_dev;
    hipError_t e;
    if (p->full) {
        e = heads ? policy_full_act_heads(p->full, p->ring, p->head, p->n, frame_dev, frame_stride, actions_dev, action_stride, logits_dev, sample, values_dev,
                                          logp_dev, st)
                  : policy_full_act(p->full, p->ring, p->head, p->n, frame_dev, frame_stride, actions_dev, action_stride, logits_dev, sample, st);
    } else {
        HIP_TRY(hipMemsetAsync(p->ticket, 0, sizeof(unsigned), st));
        // The matrix-pipe kernel, conv1 as three exact bf16 products per tap (430 us at 65 536 envs).  Profiling build only
        // (CRL_POLICY_MFMA): 1 = the same kernel with conv1 on the fp32 matrix instruction (757 us), 0 = the packed-FMA kernel of
        // round 1 (725-805 us, pong_policy_packed.inc).  The rollout launch has the one kernel.
        static const int use_mfma = CRL_ABL(getenv("CRL_POLICY_MFMA") != nullptr) ? atoi(getenv("CRL_POLICY_MFMA")) : 3;
        const HeadArgs H{p->raw + kLightWc, p->raw + kLightBc, values_dev, logp_dev};
        if (heads)
            e = policy_mfma_launch(true, p->raw, p->ring, p->head, frame_dev, frame_stride, actions_dev, action_stride, logits_dev, p->n, p->cus, p->ticket,
                                   nullptr, nullptr, sample, &H, st);
        else
#ifdef CRL_ABLATION
            if (!packed_policy_act(p->packed, use_mfma, p->ring, p->head, p->n, p->cus, frame_dev, frame_stride, actions_dev, action_stride, logits_dev,
                                   p->ticket, p->sampling, S, st, &e))
#endif
            e = policy_mfma_launch(use_mfma == 3, p->raw, p->ring, p->head, frame_dev, frame_stride, actions_dev, action_stride, logits_dev, p->n, p->cus,
                                   p->ticket, nullptr, nullptr, sample, nullptr, st);
    }
    if (e != hipSuccess) return crl_fail(CRL_EHIP, "%s: %s", who, hipGetErrorString(e));
    p->head = (p->head + 1) & 3;
    return CRL_OK;
}

int crl_policy_act(crl_policy *p, const uint8_t *frame_dev, int64_t frame_stride, int32_t *actions_dev, int64_t action_stride,
                   float *logits_dev, void *stream) {
    return policy_act("crl_policy_act", p, frame_dev, frame_stride, nullptr, actions_dev, action_stride, logits_dev, nullptr, nullptr, stream);
}

int crl_policy_act_rollout(crl_policy *p, const uint8_t *frame_dev, int64_t frame_stride, const uint8_t *reset_dev, int32_t *actions_dev,
                           int64_t action_stride, float *logits_dev, float *values_dev, float *logp_dev, void *stream) {
    return policy_act("crl_policy_act_rollout", p, frame_dev, frame_stride, reset_dev, actions_dev, action_stride, logits_dev, values_dev, logp_dev,
                      stream);
}

int crl_policy_set_critic(crl_policy *p, const float *critic_w, const float *critic_b) {
    crl_fail_no_ctx();
    if (!p || !critic_w || !critic_b) return crl_fail(CRL_EINVAL, "crl_policy_set_critic: null argument");
    HIP_TRY(hipSetDevice(p->device));
    std::vector<float> c((size_t)(p->full ? policy_full_critic_floats() : kLightCriticFloats), 0.f);
    float *dev;
    if (p->full) {
        policy_full_pack_critic(c.data(), critic_w, critic_b);
        dev = policy_full_blob(p->full) + policy_full_blob_floats();
    } else {
        policy_light_pack_critic(c.data(), critic_w, critic_b);
        dev = p->raw + kLightRawFloats;
    }
    HIP_TRY(hipMemcpy(dev, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
    p->critic = true;
    return CRL_OK;
}

int crl_policy_load_weights(crl_policy *p, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b, const float *conv3_w,
                            const float *conv3_b, const float *actor_w, const float *actor_b, const float *critic_w, const float *critic_b, void *stream) {
    crl_fail_no_ctx();
    if (!p || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !actor_w || !actor_b || !critic_w != !critic_b || !conv3_w != !conv3_b)
        return crl_fail(CRL_EINVAL, "crl_policy_load_weights: null argument (only the conv3 pair and the critic pair may be null, each as a pair)");
    if (!p->full != !conv3_w)
        return crl_fail(CRL_EINVAL, "crl_policy_load_weights: %s", p->full ? "a full-size policy needs conv3" : "a LightActorCritic policy has no conv3: pass null");
    const size_t actor_floats = p->full ? (size_t)policy_full_blob_floats() : (size_t)kLightRawFloats;
    const size_t critic_floats = p->full ? (size_t)policy_full_critic_floats() : (size_t)kLightCriticFloats;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(weight_stage_begin(p->stage, actor_floats + critic_floats));
    p->stage.host[actor_floats - 1] = 0.f;  // (the pads behind the two biases)
    for (size_t i = critic_floats - 3; i < critic_floats; i++) p->stage.host[actor_floats + i] = 0.f;
    if (p->full) {
        policy_full_pack(p->stage.host, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, actor_w, actor_b);
        if (critic_w) policy_full_pack_critic(p->stage.host + actor_floats, critic_w, critic_b);
    } else {
        policy_light_pack(p->stage.host, conv1_w, conv1_b, conv2_w, conv2_b, actor_w, actor_b);
        if (critic_w) policy_light_pack_critic(p->stage.host + actor_floats, critic_w, critic_b);
    }
    HIP_TRY(weight_stage_send(p->stage, p->full ? policy_full_blob(p->full) : p->raw, actor_floats + (critic_w ? critic_floats : 0), (hipStream_t)stream));
    if (critic_w) p->critic = true;
    return CRL_OK;
}

int crl_policy_load_weights_dev(crl_policy *p, const float *blob_dev, void *stream) {
    crl_fail_no_ctx();
    if (!p || !blob_dev) return crl_fail(CRL_EINVAL, "crl_policy_load_weights_dev: null argument");
    if (p->full) return crl_fail(CRL_EINVAL, "crl_policy_load_weights_dev: a full-size policy; the blob is a LightActorCritic's");
    HIP_TRY(hipMemcpyAsync(p->raw, blob_dev, (size_t)(kLightRawFloats + kLightCriticFloats) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    p->critic = true;
    return CRL_OK;
}

int crl_policy_load_full_dev(crl_policy *p, const float *blob_dev, void *stream) {
    crl_fail_no_ctx();
    if (!p || !blob_dev) return crl_fail(CRL_EINVAL, "crl_policy_load_full_dev: null argument");
    if (!p->full) return crl_fail(CRL_EINVAL, "crl_policy_load_full_dev: a LightActorCritic policy; the blob is a full-size network's");
    HIP_TRY(hipMemcpyAsync(policy_full_blob(p->full), blob_dev, (size_t)(policy_full_blob_floats() + policy_full_critic_floats()) * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    p->critic = true;
    return CRL_OK;
}

// crl_policy_set_sampling (`who`, calls 0) and crl_policy_resume_sampling
static int policy_set_sampling(const char *who, crl_policy *p, float temperature, float epsilon, uint64_t seed, int64_t env_id_base, uint32_t calls) {
    crl_fail_no_ctx();
    SampleArgs S{};
    if (int rc = sample_args_from(temperature, epsilon, who, &S)) return rc;
    if (!p || env_id_base < 0) return crl_fail(CRL_EINVAL, "%s: null policy or a negative env_id_base", who);
    S.seed = seed, S.id_base = env_id_base, S.n = calls;
    p->S = S;
    p->temperature = temperature, p->epsilon = epsilon;
    p->sampling = sample_active(S);
    return CRL_OK;
}

int crl_policy_set_sampling(crl_policy *p, float temperature, float epsilon, uint64_t seed, int64_t env_id_base) {
    return policy_set_sampling("crl_policy_set_sampling", p, temperature, epsilon, seed, env_id_base, 0u);
}

int crl_policy_resume_sampling(crl_policy *p, float temperature, float epsilon, uint64_t seed, int64_t env_id_base, uint32_t calls) {
    return policy_set_sampling("crl_policy_resume_sampling", p, temperature, epsilon, seed, env_id_base, calls);
}

int crl_policy_get_sampling(crl_policy *p, float *temperature, float *epsilon, uint64_t *seed, int64_t *env_id_base, uint32_t *calls) {
    crl_fail_no_ctx();
    if (!p) return crl_fail(CRL_EINVAL, "crl_policy_get_sampling: null policy");
    if (temperature) *temperature = p->temperature;
    if (epsilon) *epsilon = p->epsilon;
    if (seed) *seed = p->S.seed;
    if (env_id_base) *env_id_base = p->S.id_base;
    if (calls) *calls = p->S.n;
    return CRL_OK;
}

int crl_policy_get_blob(crl_policy *p, float *blob_out_host, int64_t blob_floats, int32_t *has_critic_out, void *stream) {
    crl_fail_no_ctx();
    if (!p || !blob_out_host) return crl_fail(CRL_EINVAL, "crl_policy_get_blob: null argument");
    const int64_t floats = p->full ? policy_full_blob_floats() + policy_full_critic_floats() : (int64_t)(kLightRawFloats + kLightCriticFloats);
    if (blob_floats != floats)
        return crl_fail(CRL_EINVAL, "crl_policy_get_blob: blob_floats %lld, but this policy's blob holds %lld", (long long)blob_floats, (long long)floats);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(blob_out_host, p->full ? policy_full_blob(p->full) : p->raw, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (has_critic_out) *has_critic_out = p->critic ? 1 : 0;
    return CRL_OK;
}

int crl_policy_get_stack(crl_policy *p, uint8_t *stack_out_dev, void *stream) { return ring_copy_stack("crl_policy_get_stack", p, stack_out_dev, 0, stream); }
int crl_policy_set_stack(crl_policy *p, const uint8_t *stack_in_dev, void *stream) { return ring_copy_stack("crl_policy_set_stack", p, stack_in_dev, 1, stream); }

}  // extern "C"

// pong_policy_packed.inc -- the packed-FMA LightActorCritic kernel of round 1, superseded by pong_policy_mfma_kernel: included by
// pong_policy.hip in the profiling build only (-DCRL_ABLATION), which launches it under CRL_POLICY_MFMA=0 for A/B.
// One kernel per call: u8 frames in, int32 actions out; nothing else touches HBM but the 7 KB
// stack per env.  The two convolutions fuse exactly because conv2 is 2x2 with stride 2: each of the
// 10x10 conv2 positions owns its 2x2 block of conv1 outputs (16 channels) and its 6x6x4 input
// patch.  One lane per conv2 position; a workgroup (256 threads) takes five envs at a time = 500
// positions in two passes:
//   conv1: 4 positions x 16 channels x 64 taps = 4 096 FMAs per lane
//   conv2: 16 channels x 64 taps                = 1 024 FMAs per lane
//   actor: 3 x 16 per lane, then a fixed-shape sum over the 100 lanes of an env in LDS
// = 516 800 FMAs per env, fp32 on the vector pipes as v_pk_fma_f32 (output channels in pairs, weights
// uniform in SGPRs): bf16/fp8 MFMA would change which action wins in close calls, the reference is
// fp32.  Roofline: 65 536 envs x 1.03 MFLOP = 67.7 GFLOP per call against 157.3 TFLOP/s packed fp32
// (measured issue rate on this chip 134-142; plain v_fma_f32 76.6).  DESIGN.md 4c has the history.

static constexpr int kEnvsPerWg = 5;
static constexpr int kPolicyThreads = 256;
static constexpr int kPasses = 2;                      // 500 positions per group over 256 lanes

// Output channels are processed in PAIRS (2p, 2p + 1) so that the multiply-adds are v_pk_fma_f32
// (two fp32 FMAs per lane per issue): weights are stored as (w[2p], w[2p + 1]) pairs, uniform per
// wavefront (scalar loads), the activation is broadcast to both halves.
struct PolicyWeights {
    const float *stream;  // conv weights in consumption order, 16 batches of 16 pairs per channel pair:
                          //   [cp 8][ conv1 [ic 4][ky 4][kx 4] | conv2 [oc pair 8][ic half 2][k 4] ] pairs, + one batch of padding
    const float *b1;      // [16]
    const f2 *b2;         // [8]
    const float *wa;      // [3][1600]      actor_linear.weight
    const float *ba;      // [3]
};

// A batch of 16 weight pairs in 32 SGPRs.  The compiler puts s_load + s_waitcnt lgkmcnt(0) right in front of
// every use (scalar loads return out of order, so it can only wait for all of them): ~200 cycles exposed per 16
// FMAs.  Here the NEXT batch is requested before the current one is consumed, and the wait sits one batch later.
typedef float v16 __attribute__((ext_vector_type(16)));
struct WBatch {
    v16 a, b;
};
__device__ inline void wbatch_request(WBatch &w, const float *p) {
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40" : "=&s"(w.a), "=&s"(w.b) : "s"(p) : "memory");
}
__device__ inline void wbatch_wait(WBatch &w) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(w.a), "+s"(w.b)); }
// Pins a batch's FMAs between the volatile request / wait statements around it (plain asm statements with no
// dependence on them may otherwise be scheduled across, which puts every wait right behind its own request).
__device__ inline void fence4(f2 &a, f2 &b, f2 &c, f2 &d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
__device__ inline void fence2(f2 &a, f2 &b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ inline f2 wbatch_get(const WBatch &w, int i) {  // i: compile-time constant
    return i < 8 ? f2{w.a[2 * i], w.a[2 * i + 1]} : f2{w.b[2 * (i - 8)], w.b[2 * (i - 8) + 1]};
}

// acc += w * broadcast(x.lo) / broadcast(x.hi): the compiler materialises a broadcast operand as a second
// register pair (doubling the 144 input registers), the instruction can select the half itself (op_sel).
__device__ inline void pk_fma_lo(f2 &acc, f2 w, f2 x) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "s"(w), "v"(x));
}
__device__ inline void pk_fma_hi(f2 &acc, f2 w, f2 x) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "s"(w), "v"(x));
}
__device__ inline void pk_fma_sel(f2 &acc, f2 w, f2 x, int half) {  // `half` is a compile-time constant after unrolling
    if (half) pk_fma_hi(acc, w, x);
    else pk_fma_lo(acc, w, x);
}
__device__ inline f2 relu2(f2 v) { return f2{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f)}; }

// a group's rings and frames into LDS: group_request_m of pong_policy.hip (where the LDS-DMA is explained) for five envs and four wavefronts
__device__ inline void group_request(uint8_t *shbuf, const uint8_t *__restrict__ ring, int head, const uint8_t *__restrict__ frame,
                                     int64_t frame_stride, int64_t env0, int envs_here, int wave, int lane) {
    for (int s = wave; s < kEnvsPerWg * 3; s += kPolicyThreads / 64) {
        const int fe = s / 3, j = s - fe * 3;
        if (fe >= envs_here) continue;
        const int pp = (head + 1 + j) & 3;
        const uint8_t *src = ring + (env0 + fe) * (int64_t)kRingBytes + pp * kPlanePad;
        uint8_t *dst = shbuf + (fe * CRL_POLICY_STACK + pp) * kPlanePad;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int c = half * 64 + lane;
            if (c < kPlaneChunks) lds_dma_b128(src + c * 16, lds_addr(dst + half * 1024));
        }
    }
    for (int s = wave; s < kEnvsPerWg * 7; s += kPolicyThreads / 64) {
        const int fe = s / 7, q = s - fe * 7;
        if (fe >= envs_here) continue;
        const int d = q * 64 + lane;
        const uint8_t *src = frame + (env0 + fe) * frame_stride;
        uint8_t *dst = shbuf + (fe * CRL_POLICY_STACK + head) * kPlanePad + q * 256;
        if (d < kPlaneWords) lds_dma_b32(src + d * 4, lds_addr(dst));
    }
}

// after the group's loads have landed (vmcnt(0) + barrier): the new frame also replaces plane `head` of the ring
__device__ inline void group_write_back(const uint8_t *shbuf, uint8_t *__restrict__ ring, int head, int64_t env0, int envs_here, int tid) {
    for (int i = tid; i < envs_here * kPlaneChunks; i += kPolicyThreads) {
        const int fe = i / kPlaneChunks, c = i - fe * kPlaneChunks;
        const uint4 v = reinterpret_cast<const uint4 *>(shbuf + (fe * CRL_POLICY_STACK + head) * kPlanePad)[c];
        reinterpret_cast<uint4 *>(ring + (env0 + fe) * (int64_t)kRingBytes + head * kPlanePad)[c] = v;
    }
}

// Persistent workgroups, TWO per CU, four wavefronts each (173 VGPRs leave two wavefronts per SIMD: one of each
// workgroup).  A workgroup takes groups b, b + gridDim.x, ... of five envs; per group it (1) pulls the rings and
// frames into LDS, (2) runs the 500 conv2 positions in two passes of 256 lanes, (3) reduces the logits.  Steps
// (1) and (3) and the patch gather of (2) keep the FMA pipes idle; the two workgroups of a CU drift apart, so
// one's idle phases run under the other's convolutions.  Tables that do not depend on the group (actor weights,
// biases) are staged once.
// SAMPLE: the action epilogue follows include/crl.h "sampled actions" (sample_action) instead of the plain argmax.
template <bool SAMPLE = false>
__global__ __launch_bounds__(kPolicyThreads) void pong_policy_light_kernel(PolicyWeights W, uint8_t *__restrict__ ring, int head,
                                                                           const uint8_t *__restrict__ frame, int64_t frame_stride,
                                                                           int32_t *__restrict__ actions, int64_t action_stride,
                                                                           float *__restrict__ logits_out, int64_t n, unsigned *__restrict__ ticket,
                                                                           SampleArgs S) {
    __shared__ __attribute__((aligned(16))) uint8_t sh_in[kEnvsPerWg][CRL_POLICY_STACK][kPlanePad];
    __shared__ float sh_wa[3 * 1600];
    __shared__ __attribute__((aligned(8))) float sh_b2[16];  // conv2.bias; actor bias: no VMEM loads inside the loop,
    __shared__ float sh_ba[4];                               // a wait on one would also wait on the group in flight
    __shared__ float sh_part[kEnvsPerWg * kPos][3];
    __shared__ float sh_grp[kEnvsPerWg][3][4];
    __shared__ float sh_logit[kEnvsPerWg][3];
    const int tid = threadIdx.x;
    const int64_t ngroups = (n + kEnvsPerWg - 1) / kEnvsPerWg;

    if (tid < 16) sh_b2[tid] = reinterpret_cast<const float *>(W.b2)[tid];
    if (tid < 3) sh_ba[tid] = W.ba[tid];
    for (int i = tid; i < 3 * 1600; i += kPolicyThreads) sh_wa[i] = W.wa[i];
    // The conv1 bias is fetched with v_readlane from lanes 0..15 of the wavefront, so there is NO divergent
    // branch around the convolutions: every wavefront that runs the loop must hold it in those lanes (a
    // wavefront whose live lanes stop before lane 15 would read registers that were never written).  Idle
    // lanes (the last 12 of the workgroup, envs past the end) redo a valid position and drop the result.
    const float b1i = W.b1[tid & 15];  // lane l of every wavefront holds conv1.bias[l & 15]
    const int b1lane = __float_as_int(b1i);
    const int wave = tid >> 6, lane = tid & 63;
    __syncthreads();
    // Groups are handed out by a ticket counter, not b, b + grid, ...: the SIMDs favour their OLDEST wavefront, so the
    // workgroup that reached a CU first runs about twice as fast as its co-resident (cycle-counter timelines: 48 k vs
    // 96 k cycles per group) and a static split leaves the slow half to finish alone.
    __shared__ unsigned sh_ticket;
    for (int64_t g = blockIdx.x; g < ngroups;) {
        const int64_t env0 = g * kEnvsPerWg;
        const int envs_here = (int)((n - env0) < kEnvsPerWg ? (n - env0) : kEnvsPerWg);
        if (tid == 0) sh_ticket = atomicAdd(ticket, 1u);
        group_request(&sh_in[0][0][0], ring, head, frame, frame_stride, env0, envs_here, wave, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's share has landed
        __syncthreads();                                    // ... everybody's has
        const int64_t g_next = (int64_t)gridDim.x + sh_ticket;  // rewritten only after this iteration's last barrier
        group_write_back(&sh_in[0][0][0], ring, head, env0, envs_here, tid);
      for (int pass = 0; pass < kPasses; pass++) {
        const int task = pass * kPolicyThreads + tid;
        const int e = task < kEnvsPerWg * kPos ? task / kPos : kEnvsPerWg - 1;
        const int pos = task < kEnvsPerWg * kPos ? task - e * kPos : 0;
        const int y2 = pos / 10, x2 = pos - y2 * 10;
        const bool live = task < kEnvsPerWg * kPos && env0 + e < n;
        float l0 = 0.f, l1 = 0.f, l2 = 0.f;
        {
            // The 6x6x4 patch as floats, columns (2k, 2k + 1) in one register pair.  Measured with the cycle counter:
            // this gather, not the FMAs next to it, was a quarter of the kernel when it was 72 ds_read_u16 + 144
            // look-ups in a b/255 table per lane -- LDS-pipe bound (eight wavefronts of a CU share it), not latency
            // bound.  Now two ALIGNED dwords per 6-byte row piece in one ds_read2_b32 (the piece starts on a multiple
            // of 4 for even r and 2 bytes after one for odd r -- known at compile time; an unaligned ds_read_b64 is no
            // faster than the 216 small reads) and the division on the vector pipes: q = b * fl(1/255) + one
            // FMA-corrected Newton step = correctly rounded b / 255.0f for every byte (Markstein), i.e. the
            // reference's x / 255 bit for bit.
            f2 in[4][6][3];
            const f2 rcp = f2{1.0f / 255.0f, 1.0f / 255.0f}, m255 = f2{-255.0f, -255.0f};
#pragma unroll
            for (int ic = 0; ic < 4; ic++)
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    // logical plane ic (oldest first) is ring plane (head + 1 + ic) & 3; bytes read past the piece stay
                    // inside the padded plane
                    const uint8_t *row = &sh_in[e][(head + 1 + ic) & 3][(4 * y2 + r) * kDim + 4 * x2];
                    const uint32_t *p32 = reinterpret_cast<const uint32_t *>(row - 2 * (r & 1));
                    uint32_t w0 = p32[0], w1 = p32[1];
                    if (r & 1) w0 = (w0 >> 16) | (w1 << 16), w1 >>= 16;
                    const f2 b[3] = {f2{(float)(w0 & 255u), (float)((w0 >> 8) & 255u)}, f2{(float)((w0 >> 16) & 255u), (float)(w0 >> 24)},
                                     f2{(float)(w1 & 255u), (float)((w1 >> 8) & 255u)}};
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const f2 q = b[k] * rcp;
                        const f2 rem = __builtin_elementwise_fma(q, m255, b[k]);
                        in[ic][r][k] = __builtin_elementwise_fma(rem, rcp, q);
                    }
                }
            f2 acc[8];  // conv2 accumulators, output channels (2p, 2p + 1)
#pragma unroll
            for (int p = 0; p < 8; p++) acc[p] = reinterpret_cast<const f2 *>(sh_b2)[p];
            const float *wp = W.stream;
            WBatch wa_, wb_;
            wbatch_request(wa_, wp);
#define CRL_CONV1_BATCH(WB, IC)                                                  \
    _Pragma("unroll") for (int ky = 0; ky < 4; ky++)                             \
        _Pragma("unroll") for (int kx = 0; kx < 4; kx++) {                       \
        const f2 w = wbatch_get(WB, ky * 4 + kx);                                \
        pk_fma_sel(h00, w, in[IC][ky][kx >> 1], kx & 1);                         \
        pk_fma_sel(h01, w, in[IC][ky][(kx >> 1) + 1], kx & 1);                   \
        pk_fma_sel(h10, w, in[IC][ky + 2][kx >> 1], kx & 1);                     \
        pk_fma_sel(h11, w, in[IC][ky + 2][(kx >> 1) + 1], kx & 1);               \
    }                                                                            \
    fence4(h00, h01, h10, h11);
#define CRL_CONV2_BATCH(WB, J)                                                   \
    {                                                                            \
        f2 a0 = acc[2 * (J)], a1 = acc[2 * (J) + 1];                             \
        pk_fma_lo(a0, wbatch_get(WB, 0), h00);                                   \
        pk_fma_lo(a1, wbatch_get(WB, 8), h00);                                   \
        pk_fma_lo(a0, wbatch_get(WB, 1), h01);                                   \
        pk_fma_lo(a1, wbatch_get(WB, 9), h01);                                   \
        pk_fma_lo(a0, wbatch_get(WB, 2), h10);                                   \
        pk_fma_lo(a1, wbatch_get(WB, 10), h10);                                  \
        pk_fma_lo(a0, wbatch_get(WB, 3), h11);                                   \
        pk_fma_lo(a1, wbatch_get(WB, 11), h11);                                  \
        pk_fma_hi(a0, wbatch_get(WB, 4), h00);                                   \
        pk_fma_hi(a1, wbatch_get(WB, 12), h00);                                  \
        pk_fma_hi(a0, wbatch_get(WB, 5), h01);                                   \
        pk_fma_hi(a1, wbatch_get(WB, 13), h01);                                  \
        pk_fma_hi(a0, wbatch_get(WB, 6), h10);                                   \
        pk_fma_hi(a1, wbatch_get(WB, 14), h10);                                  \
        pk_fma_hi(a0, wbatch_get(WB, 7), h11);                                   \
        pk_fma_hi(a1, wbatch_get(WB, 15), h11);                                  \
        fence2(a0, a1);                                                          \
        acc[2 * (J)] = a0, acc[2 * (J) + 1] = a1;                                \
    }
#define CRL_STEP(CUR, NXT, OFS, WORK)   \
    wbatch_wait(CUR);                   \
    wbatch_request(NXT, wp + (OFS));    \
    WORK
            for (int cp = 0; cp < 8; cp++) {  // conv1 output channels (2cp, 2cp + 1) == conv2 input channels
                const f2 bias = f2{__int_as_float(__builtin_amdgcn_readlane(b1lane, 2 * cp)),
                                   __int_as_float(__builtin_amdgcn_readlane(b1lane, 2 * cp + 1))};
                f2 h00 = bias, h01 = bias, h10 = bias, h11 = bias;
                CRL_STEP(wa_, wb_, 32, CRL_CONV1_BATCH(wa_, 0))
                CRL_STEP(wb_, wa_, 64, CRL_CONV1_BATCH(wb_, 1))
                CRL_STEP(wa_, wb_, 96, CRL_CONV1_BATCH(wa_, 2))
                CRL_STEP(wb_, wa_, 128, CRL_CONV1_BATCH(wb_, 3))
                h00 = relu2(h00), h01 = relu2(h01), h10 = relu2(h10), h11 = relu2(h11);
                CRL_STEP(wa_, wb_, 160, CRL_CONV2_BATCH(wa_, 0))
                CRL_STEP(wb_, wa_, 192, CRL_CONV2_BATCH(wb_, 1))
                CRL_STEP(wa_, wb_, 224, CRL_CONV2_BATCH(wa_, 2))
                CRL_STEP(wb_, wa_, 256, CRL_CONV2_BATCH(wb_, 3))  // the next channel pair's first batch (padding after the last)
                wp += 256;
            }
            wbatch_wait(wa_);  // drain the padding request
#undef CRL_STEP
#undef CRL_CONV1_BATCH
#undef CRL_CONV2_BATCH
#pragma unroll
            for (int oc = 0; oc < 16; oc++) {
                const float f = fmaxf((oc & 1) ? acc[oc >> 1].y : acc[oc >> 1].x, 0.f);
                l0 = __builtin_fmaf(sh_wa[0 * 1600 + oc * kPos + pos], f, l0);
                l1 = __builtin_fmaf(sh_wa[1 * 1600 + oc * kPos + pos], f, l1);
                l2 = __builtin_fmaf(sh_wa[2 * 1600 + oc * kPos + pos], f, l2);
            }
        }
        if (live) sh_part[task][0] = l0, sh_part[task][1] = l1, sh_part[task][2] = l2;
      }
        __syncthreads();
        // fixed-shape sum over the 100 positions of an env (4 groups of 25, then the 4 groups): the result
        // does not depend on scheduling
        if (tid < kEnvsPerWg * 12) {
            const int pe = tid / 12, r = tid - pe * 12, a = r >> 2, grp = r & 3;
            float s = 0.f;
#pragma unroll
            for (int p = 0; p < 25; p++) s += sh_part[pe * kPos + grp * 25 + p][a];
            sh_grp[pe][a][grp] = s;
        }
        __syncthreads();
        if (tid < kEnvsPerWg * 3) {
            const int pe = tid / 3, a = tid - pe * 3;
            sh_logit[pe][a] = sh_ba[a] + ((sh_grp[pe][a][0] + sh_grp[pe][a][1]) + (sh_grp[pe][a][2] + sh_grp[pe][a][3]));
        }
        __syncthreads();
        if (tid < kEnvsPerWg && env0 + tid < n)
            action_epilogue<SAMPLE>(S, env0 + tid, sh_logit[tid][0], sh_logit[tid][1], sh_logit[tid][2], actions, action_stride, logits_out);
        __syncthreads();  // sh_logit / sh_in are rewritten by the next group
        g = g_next;
    }
}

// ---- host: the weight stream of a crl_policy (owned through W.stream) and the launch
static hipError_t packed_policy_create(PolicyWeights &W, const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b,
                                       const float *actor_w, const float *actor_b) {
    // one blob: stream 2048 + 32 pad | b1 16 | b2 16 | wa 4800 | ba 3 (+ pad)
    std::vector<float> blob(2080 + 16 + 16 + 4800 + 4, 0.f);
    float *st = blob.data(), *b1 = st + 2080, *b2 = b1 + 16, *wa = b2 + 16, *ba = wa + 4800;
    for (int oc = 0; oc < 16; oc++)  // torch conv1 [oc][tap] -> [oc / 2][tap][oc & 1] at the head of block oc / 2
        for (int k = 0; k < 64; k++) st[(oc >> 1) * 256 + k * 2 + (oc & 1)] = conv1_w[oc * 64 + k];
    for (int oc = 0; oc < 16; oc++)  // torch conv2 [oc][ic][ky][kx] -> block ic / 2: [oc / 2][ic & 1][k][oc & 1]
        for (int ic = 0; ic < 16; ic++)
            for (int k = 0; k < 4; k++)
                st[(ic >> 1) * 256 + 128 + (((oc >> 1) * 2 + (ic & 1)) * 4 + k) * 2 + (oc & 1)] = conv2_w[(oc * 16 + ic) * 4 + k];
    memcpy(b1, conv1_b, 16 * sizeof(float));
    memcpy(b2, conv2_b, 16 * sizeof(float));
    memcpy(wa, actor_w, 4800 * sizeof(float));
    memcpy(ba, actor_b, 3 * sizeof(float));
    float *base = nullptr;  // hipMalloc: 256-byte aligned, so every 64-byte batch is aligned
    hipError_t e = hipMalloc(&base, blob.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(base, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
    W.stream = base, W.b1 = base + 2080, W.b2 = reinterpret_cast<const f2 *>(base + 2096);
    W.wa = base + 2112, W.ba = base + 6912;
    return e;
}

// The one entry of crl_policy_act.  False: this process did not select the packed-FMA kernel (CRL_POLICY_MFMA is 1, 3 or unset)
// and nothing was launched; true: *err is the launch's outcome.  `ticket` is zeroed by the caller.
static bool packed_policy_act(const PolicyWeights &W, int use_mfma, uint8_t *ring, int head, int64_t n, int cus, const uint8_t *frame_dev,
                              int64_t frame_stride, int32_t *actions_dev, int64_t action_stride, float *logits_dev, unsigned *ticket, bool sampling,
                              const SampleArgs &S, hipStream_t st, hipError_t *err) {
    if (use_mfma == 1 || use_mfma == 3) return false;
    const int64_t groups = (n + kEnvsPerWg - 1) / kEnvsPerWg;
    const unsigned grid = (unsigned)(groups < 2 * cus ? groups : 2 * cus);  // persistent: two workgroups per CU
    const auto kernel = sampling ? pong_policy_light_kernel<true> : pong_policy_light_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPolicyThreads), 0, st, W, ring, head, frame_dev, frame_stride, actions_dev, action_stride, logits_dev, n, ticket,
                       S);
    *err = hipGetLastError();
    return true;
}

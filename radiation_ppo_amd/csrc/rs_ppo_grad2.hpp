// rs_ppo_grad2.hpp -- K7 v2: the fused PPO loss+gradient pass with 32 samples per wave and TWO waves per SIMD.
//
// v1 (rs_ppo_grad_kernel) gives every wave 64 samples and ~500 registers, i.e. one wave per SIMD: the VALU/LDS
// phases of a group (tanh, output layer, loss, tile staging) cannot hide behind the MFMA phases because an
// in-order wave has no second wave to interleave with -- rocprof shows the matrix pipe 55-60 % busy.  v2 halves
// the transient state (one 32-sample tile per wave: H1, H2, dH1 are 32 registers each), keeps the whole kernel
// under 256 registers, and launches 512-thread workgroups = 8 waves per CU = 2 per SIMD, so the hardware
// overlaps one wave's VALU/LDS work with the other's MFMAs.
//
// Lane mapping (v_mfma_f32_32x32x2_f32): lane l = (c = l&31, h = l>>5); both lanes (c, 0) and (c, 1) belong to
// sample c of the group and hold the hidden units 32*it + kappa(r, h) of that sample, so no partner exchange is
// needed for the inputs or for dz; per-sample scalars are computed redundantly in both lanes.
#pragma once
#include "rs_mlp.hpp"

#define RS_T2 33                                   // row stride of the 32-sample LDS tiles (floats)

// Diagnostic build only (-DRS_K7_STAMPS, scripts/k7_stamps.py): s_memtime stamps at the phase boundaries of the sample-group
// loop, summed per wave in scalar registers and added to a table no other code reads; slot 12 is the prologue (kernel entry to
// the first trip), slot 13 the epilogue (last trip to the end of the kernel).  The product build contains none of it.
#ifdef RS_K7_STAMPS
#define RS_K7_NPH 16
__device__ unsigned long long rs_k7_stamp_table[2][RS_K7_NPH];
#define RS_STAMP_ENTRY const unsigned long long st_rt0 = __builtin_amdgcn_s_memrealtime(); const unsigned long long st_t0 = rs_k7_now();
#define RS_STAMP_DECL unsigned long long st_acc[RS_K7_NPH] = {0}; unsigned long long st_last = rs_k7_now(); st_acc[12] = st_last - st_t0;
// end of the kernel: the epilogue's cycles, the 100 MHz ticks of the whole kernel (in-kernel clock = cycles / ticks * 100 MHz)
#define RS_STAMP_EXIT(net) do { RS_STAMP(13); if ((threadIdx.x & 63) == 0) { st_acc[14] = __builtin_amdgcn_s_memrealtime() - st_rt0; \
                           for (int q = 0; q < RS_K7_NPH; ++q) atomicAdd(&rs_k7_stamp_table[net][q], st_acc[q]); } } while (0)
#define RS_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); asm volatile("; RS_STAMP_MARK " #i); const unsigned long long t_ = rs_k7_now(); st_acc[i] += t_ - st_last; st_last = t_; \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
__device__ __forceinline__ unsigned long long rs_k7_now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#else
#define RS_STAMP_ENTRY
#define RS_STAMP_DECL
#define RS_STAMP_EXIT(net)
// product build: a phase boundary is a scheduling fence only (A/B switch RS_K7_NO_PHASE_FENCE: hipcc is then free to move LDS
// reads, staging writes and VALU work across the phases)
#ifdef RS_K7_NO_PHASE_FENCE
#define RS_STAMP(i) do {} while (0)
#else
#define RS_STAMP(i) __builtin_amdgcn_sched_barrier(0)
#endif
#endif
// Diagnostic build only (-DRS_K7_SKEW, scripts/k7_partner_gap.py): how far apart do the waves of a workgroup leave the trip loop, and
// how long do they then wait at the epilogue's first barrier?  Three s_memtime reads per wave and launch (end of the last trip,
// release of that barrier, end of the kernel, each counted from kernel entry) and none inside the loop: no per-phase stamp, no fence,
// so the trips overlap as in the product build.  Summed per network and wave slot in a table no other code reads:
//   [0..7] loop end  [8..15] barrier release  [16..23] kernel end  [24..55] waves of slot w seen on SIMD s, at [24 + 4 w + s]
//   [56..59] loop end of wave w + 4 minus loop end of wave w, per workgroup  [60..63] the same as |.|  [64] launches  [65] 100 MHz ticks
// The loop ends cross the waves through eight LDS slots behind the progress words.
#ifdef RS_K7_SKEW
#define RS_K7_NSK 66
__device__ unsigned long long rs_k7_skew_table[2][RS_K7_NSK];
__device__ __forceinline__ unsigned long long rs_k7_clock() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#define RS_SKEW_LDS_FLOATS 16
#define RS_SKEW_ENTRY const unsigned long long sk_rt0 = __builtin_amdgcn_s_memrealtime(); const unsigned long long sk_t0 = rs_k7_clock();
#define RS_SKEW_LOOP_END(slots) const unsigned long long sk_t1 = rs_k7_clock() - sk_t0; \
    if ((threadIdx.x & 63) == 0) (slots)[threadIdx.x >> 6] = sk_t1;
#define RS_SKEW_RELEASED const unsigned long long sk_tb = rs_k7_clock() - sk_t0;
#define RS_SKEW_PAIRS(net, slots) if ((threadIdx.x & 63) == 0 && threadIdx.x < 256 && blockDim.x == 512) { \
        const long long d_ = (long long)((slots)[(threadIdx.x >> 6) + 4] - (slots)[threadIdx.x >> 6]); \
        atomicAdd(&rs_k7_skew_table[net][56 + (threadIdx.x >> 6)], (unsigned long long)d_); \
        atomicAdd(&rs_k7_skew_table[net][60 + (threadIdx.x >> 6)], (unsigned long long)(d_ < 0 ? -d_ : d_)); }
// HW_REG_HW_ID (register 4), bits 5:4 = SIMD_ID: s_getreg_b32 with simm16 = id | offset << 6 | (size - 1) << 11
#define RS_SKEW_EXIT(net) do { const unsigned long long sk_t2 = rs_k7_clock() - sk_t0; if ((threadIdx.x & 63) == 0) { \
        const int w_ = threadIdx.x >> 6; unsigned long long* T_ = rs_k7_skew_table[net]; \
        atomicAdd(&T_[w_], sk_t1); atomicAdd(&T_[8 + w_], sk_tb); atomicAdd(&T_[16 + w_], sk_t2); \
        atomicAdd(&T_[24 + 4 * w_ + (int)__builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11))], 1ull); \
        atomicAdd(&T_[65], __builtin_amdgcn_s_memrealtime() - sk_rt0); \
        if (bid == 0 && w_ == 0) atomicAdd(&T_[64], 1ull); } } while (0)
#else
#define RS_SKEW_LDS_FLOATS 0
#define RS_SKEW_ENTRY
#define RS_SKEW_LOOP_END(slots)
#define RS_SKEW_RELEASED
#define RS_SKEW_PAIRS(net, slots)
#define RS_SKEW_EXIT(net)
#endif

// Partner balance.  The two waves of a SIMD (wave slots w and w + 4 of the 512-thread workgroup) share its issue slots by priority
// first and age second, so at equal priority the older one runs ahead, ends its trips early and idles at the epilogue's barrier
// while its partner finishes alone -- for 134 us of the actor's 585 at M = 1 966 080, and a wave alone on its SIMD delivers 0.88 of the
// paired throughput (profiles/r13_k7_partner_balance_ab.txt).  Every wave therefore publishes its progress in an LDS word of its own, reads its partner's once per trip and takes priority 1 when it is
// behind (on a tie: the younger wave), priority 0 when it is ahead.  Nothing waits on the word: the read races with the partner's
// store by design (relaxed workgroup-scope atomics) and only moves issue slots between the two; which groups a wave sums, and in
// which order, does not change.  RS_K7_PRIO selects the rule for A/B builds:
//   0  none (both waves at priority 0 throughout)
//   1  progress words, compared at the top of every trip (the product build)
//   2  progress words, compared at the top of the trip and again after the loss
//   3  no LDS: bit RS_K7_PRIO_BIT of s_memtime, flipped for the younger half, read at the top of the trip
//   4  control: static priority 1 for wave slots 4..7
#ifndef RS_K7_PRIO
#define RS_K7_PRIO 1
#endif
#ifndef RS_K7_PRIO_BIT
#define RS_K7_PRIO_BIT 15
#endif
#define RS_K7_PROG_FLOATS 8                        // the eight progress words, behind the last wave's zones

#define RS_XRAW 400                                // per-wave landing zone of the group's 32 x 11 sample rows (352 floats, LDS-DMA);
                                                   // between layer 1 and the next DMA it holds the tail of the stride-36 h2^T tile and
                                                   // behind it the [12][36] dz / statistics rows, which run on into xsc (actor), or
                                                   // the dz / loss rows and a row of ones (critic)
#define RS_XSC 192                                 // per-wave landing zone of the per-sample scalars: act (32 x int64), adv, logp_old, w, ret
#define RS_G2_WAVE_FLOATS ((64 + 32) * RS_T2 + RS_XRAW + RS_XSC + 64)

__host__ __device__ constexpr int rs_grad2_lds_floats(int nout) {
    return ((rs_mlp_lds_floats(nout) + 3) & ~3) + 2 * 2 * 16 * 64 + 2 * 4 * 64 + 8 * RS_G2_WAVE_FLOATS + RS_K7_PROG_FLOATS + RS_SKEW_LDS_FLOATS;
}

// the value lane l ^ 32 holds (__shfl_xor(x, 32) without the LDS crossbar): v_permlane32_swap exchanges the upper half of its
// first operand with the lower half of its second
__device__ __forceinline__ float rs_other_half(float x, int h) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(h ? r[0] : r[1]);
}

// The element-wise chains of the group loop run on explicit pairs, registers r and r + 1 of an accumulator: v_pk_add_f32 /
// v_pk_mul_f32 / v_pk_fma_f32 do two values per issue slot (the translation unit is built without SLP packing, so nothing else
// pairs up).  Every element keeps its operations and roundings.
typedef float rs_f2 __attribute__((ext_vector_type(2)));

// rs_tanh_scaled of the 16 values of an accumulator: 1 + e and fma(-2, rcp, 1) per pair around the two v_exp_f32 / v_rcp_f32
__device__ __forceinline__ void rs_tanh_scaled16(f32x16& v) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const rs_f2 e = (rs_f2){1.0f, 1.0f} + (rs_f2){__builtin_amdgcn_exp2f(v[r]), __builtin_amdgcn_exp2f(v[r + 1])};
        const rs_f2 t = __builtin_elementwise_fma((rs_f2){-2.0f, -2.0f}, (rs_f2){__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)},
                                                  (rs_f2){1.0f, 1.0f});
        v[r] = t.x; v[r + 1] = t.y;
    }
}

// d (1 - h^2) as fma(-(d h), h, d), a pair at a time
__device__ __forceinline__ rs_f2 rs_dtanh2(rs_f2 d, rs_f2 hv) { return __builtin_elementwise_fma(-(d * hv), hv, d); }

__device__ __forceinline__ void rs_stage32(float* T, const f32x16& v, int c, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) T[rs_kappa(r, h) * RS_T2 + c] = v[r];
}

// The whole pass of one network as ONE workgroup sees it: workgroup `bid` of `nblocks`.  rs_ppo_grad2_kernel passes its launch's own
// index and grid size; rs_ppo_grad2_pair_kernel runs both networks' workgroups in one grid and hands each its index in its own half.
// No __restrict__ here: the kernels' own parameters carry it.  Repeated on this inlined function it becomes alias scopes on every
// access of the group loop, and hipcc then waits for the LDS reads in bulk (s_waitcnt lgkmcnt(0)) where it counted them down one
// MFMA operand at a time: + 1.7 % on the pass (measured, profiles/r07_update_launches_ab.txt).
template <int NOUT>
__device__ __forceinline__ void rs_ppo_grad2_body(const RsMlpParams prm, const rs_ppo_batch B, float* partial,
                                                  double* stat_partial, const int* stop,
                                                  const rs_update_state* ust, int* snap,
                                                  const int bid, const int nblocks) {
    extern __shared__ __align__(16) float smem_f[];
    // snap (fused single-GPU tail only): a copy of the update state's step count and stop flag for rs_ppo_tail_kernel, all of whose
    // workgroups read them while one of them writes the state -- the copy is what makes that free of a race without any waiting
    if (snap && bid == 0 && threadIdx.x == 0) { snap[0] = ust->adam_step; snap[1] = ust->stopped; }
    if (stop && *stop) return;
    RS_STAMP_ENTRY
    RS_SKEW_ENTRY
    RsMlpLds<NOUT> W;
    W.carve(smem_f);
    float* w2tf = smem_f + ((rs_mlp_lds_floats(NOUT) + 3) & ~3);   // 16-byte aligned; [2 it][2 kt][4 r4][64 lanes][4]: W2[32kt + kappa(r, l>>5)][32it + (l&31)]
    float* w3tf = w2tf + 2 * 2 * 16 * 64;               // [2 it][4 s][64]:        W3[2s + (l>>5)][32it + (l&31)]
    // wave id as a SCALAR: the per-wave LDS bases below then live in SGPRs (and M0 for the LDS-DMA) instead of VGPRs
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int l15 = lane & 15, l4 = lane >> 4;
    float* Qt = w3tf + 2 * 4 * 64 + wid * RS_G2_WAVE_FLOATS;   // [64][33]  h^T tile (h2 for dW3, then h1 for dW2)
    float* Pt = Qt + 64 * RS_T2;                               // [32][33]  dpre^T half tile
    float* xraw = Pt + 32 * RS_T2;                             // [32][11]  the group's sample rows as they lie in HBM (LDS-DMA target)
    float* xsc = xraw + RS_XRAW;                               // [192]     the group's per-sample scalars (LDS-DMA target)
    float* dbl = xsc + RS_XSC;                                 // [64]      db2 accumulators of this wave
    // [8] progress words, one per wave: outside every zone the trip loop or the look-ahead DMA writes
    int* prog = reinterpret_cast<int*>(w3tf + 2 * 4 * 64 + 8 * RS_G2_WAVE_FLOATS);
#ifdef RS_K7_SKEW
    unsigned long long* sk_slots = reinterpret_cast<unsigned long long*>(prog + RS_K7_PROG_FLOATS);      // [8] loop ends
#endif
    // Fragment fill, one pass per array and ONE barrier.  Not RsMlpLds::fill (the forward kernel's): K7 wants W2 in the b128 form
    // below, the layer-1 bias inside w1f, and never reads W.b1.
    // layer-1 fragments with the bias in the padded input column k = 11 (k-step 5, upper lane half)
    float* w1b = W.w1f;
    for (int i = threadIdx.x; i < 2 * 6 * 64; i += blockDim.x) {
        const int l = i & 63, s = (i >> 6) % 6, it = i / (6 * 64);
        const int row = 32 * it + (l & 31), k = 2 * s + (l >> 5);
        w1b[i] = RS_TANH_PRESCALE * ((k < RS_IN) ? prm.w1[row * RS_IN + k] : prm.b1[row]);
    }
    // W2 fragments for the matrix pipe, four consecutive k-steps per lane contiguous ([it][kt][r / 4][lane][r % 4]): one
    // ds_read_b128 feeds four MFMAs (an LDS read instruction costs the wave ~13 issue cycles whatever its width).  w2tf is
    // the transpose (dh1 = W2^T dpre2), W.w2f the forward copy with the tanh prescale.
    for (int i = threadIdx.x; i < 2 * 2 * 16 * 64; i += blockDim.x) {
        const int ri = i & 3, l = (i >> 2) & 63, r4 = (i >> 8) & 3, kt = (i >> 10) & 1, it = i >> 11;
        const int r = 4 * r4 + ri;
        w2tf[i] = prm.w2[(32 * kt + rs_kappa(r, l >> 5)) * RS_HID + 32 * it + (l & 31)];
        W.w2f[i] = RS_TANH_PRESCALE * prm.w2[(32 * it + (l & 31)) * RS_HID + 32 * kt + rs_kappa(r, l >> 5)];
    }
    for (int i = threadIdx.x; i < 2 * 4 * 64; i += blockDim.x) {
        int l = i & 63, sq = (i >> 6) & 3, it = i >> 8;
        int o = 2 * sq + (l >> 5);
        w3tf[i] = (o < NOUT) ? prm.w3[o * RS_HID + 32 * it + (l & 31)] : 0.0f;
    }
    // The output layer's weights.  Critic: [2 h][32 q] as in RsMlpLds.  Actor: the same values chunk-major, [8 b][2 h][8 o][4 j] with
    // q = 4 b + j, because there every lane reads the row of an output of its own (A operand of the 4x4x1 chains): the 16 lanes a
    // ds_read_b128 serves together read four different rows, which lie in four neighbouring 16-byte slots here (no bank conflict;
    // 128-byte rows would put them two to a bank).
    for (int i = threadIdx.x; i < 2 * NOUT * 32; i += blockDim.x) {
        int q = i & 31, o = (i >> 5) % NOUT, hh = i / (32 * NOUT);
        if constexpr (NOUT == 8) { q = 4 * (i >> 6) + (i & 3); o = (i >> 2) & 7; hh = (i >> 5) & 1; }
        W.w3h[i] = prm.w3[o * RS_HID + 32 * (q >> 4) + rs_kappa(q & 15, hh)];
    }
    for (int i = threadIdx.x; i < 64; i += blockDim.x) W.b2[i] = RS_TANH_PRESCALE * prm.b2[i];
    for (int i = threadIdx.x; i < NOUT; i += blockDim.x) W.b3[i] = prm.b3[i];
    dbl[lane] = 0.0f;
    if (threadIdx.x < RS_K7_PROG_FLOATS) prog[threadIdx.x] = 0;
    __syncthreads();

    const int M = B.M;
    const int groups = (M + 31) / 32;
    const int wave_g = bid * 8 + wid, n_waves = nblocks * 8;

    f32x16 acc2[2][2];
    f32x4 acc1[4], acc3[2];                         // acc3: two 4x4x1 accumulators per network, see the dW3 phase
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc2[a][0][r] = 0.f; acc2[a][1][r] = 0.f; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int a = 0; a < 4; ++a) acc1[a][r] = 0.f;
        acc3[0][r] = 0.f; acc3[1][r] = 0.f;
    }
    // db3 and the loss statistics are per-sample scalars summed over samples: they ride in the dz^T rows (rows 0..NOUT-1: dz,
    // rows 8..11: kl / entropy / clip fraction / surrogate terms) and are summed by one more 4x4x1 chain per group against a B
    // operand of ones -- no per-lane accumulators, no cross-lane reduction (actor; the critic's sums ride in acc3)
    f32x4 accs;
#pragma unroll
    for (int r = 0; r < 4; ++r) accs[r] = 0.f;

    // ---- sample data of a group: the 32 x 11 rows lie contiguously in HBM (352 floats) and are copied to the wave's LDS
    // landing zone by LDS-DMA (six 256-byte wave-instructions, no registers), the per-sample scalars (action, advantage,
    // old log-prob, weight, return) by three more.  Both are fetched ONE GROUP AHEAD (issued once the landing zones are free,
    // after the dW3 phase), so no HBM latency is exposed and no register is held across the group.
    // Every wave runs the same number of trips; a trip past the last group works on clamped rows with weight 0.
    const int trips = (groups + n_waves - 1) / n_waves;
    // The rows' transfers are addressed as a wave-uniform base (SGPR pair: the group's first float) plus a 32-bit per-lane byte
    // offset, the global_load_lds_dword saddr form: no 64-bit per-lane address pair is formed or kept live across the group.
    const long x_last = (long)M * RS_IN - 1;
    auto dma_rows = [&](int g) {
        const char* gx = reinterpret_cast<const char*>(B.x + (long)g * (32 * RS_IN));
        const int lim = (int)(x_last - (long)g * (32 * RS_IN));    // tail of the last group / lanes past the 352 floats: stay in bounds
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int o = min(i * 64 + lane, lim);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gx + 4u * (unsigned)o),
                                             (__attribute__((address_space(3))) void*)(xraw + i * 64), 4, 0, 0);
        }
    };
    auto dma_scal = [&](int g) {
        // three wave-instructions: [act: 64 dwords = 32 int64] [adv | logp_old] [w | ret]; sample index clamped like the rows.
        // The critic reads neither the action nor adv / logp_old: it issues the third only.
        const int m0 = g * 32;
        const int ms = min(m0 + c, M - 1);
        if constexpr (NOUT == 8) {
            const int mi = min(m0 + (lane >> 1), M - 1);
            const int* src = reinterpret_cast<const int*>(B.act) + 2 * (size_t)mi + (lane & 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(xsc), 4, 0, 0);
        }
        if constexpr (NOUT == 8) {
            const float* src = (h ? B.logp_old : B.adv) + ms;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(xsc + 64), 4, 0, 0);
        }
        {
            const float* src = (h ? B.ret : B.w) + ms;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(xsc + 128), 4, 0, 0);
        }
    };
    {
        const int g0 = wave_g < groups ? wave_g : groups - 1;
        dma_rows(g0);
        dma_scal(g0);
    }
    // ---- critic only (NOUT == 1): its sample-group loop differs from the actor's in the sections marked `if constexpr (NOUT == 1)`.
    // w3v: the 32 output weights of the units this lane holds, W3[0][32 kt + kappa(r, h)] at [16 kt + r], read once as eight b128 and
    // kept across the trips (output layer and dh2 = W3^T dz both use them).  db2r: the db2 sums of units 32 it + c, in every lane.
    float w3v[NOUT == 1 ? 32 : 1], db2r[2] = {0.0f, 0.0f};
    if constexpr (NOUT == 1) {
        const float4* wrow = reinterpret_cast<const float4*>(W.w3h + h * 32);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const float4 t = wrow[b];
            w3v[4 * b + 0] = t.x; w3v[4 * b + 1] = t.y; w3v[4 * b + 2] = t.z; w3v[4 * b + 3] = t.w;
        }
    }
    // partner balance (see RS_K7_PRIO): publish `at`, read the partner's word once, act on whatever is there
    auto balance = [&](const int at) {
#if RS_K7_PRIO == 1 || RS_K7_PRIO == 2
        if (lane == 0) __hip_atomic_store(prog + wid, at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int theirs = __builtin_amdgcn_readfirstlane(__hip_atomic_load(prog + (wid ^ 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        // s_setprio is scalar and ignores EXEC: the condition is made of SGPR values only (wid and theirs come from readfirstlane)
        // behind the partner, or level with it and the younger of the two (wid >> 2 is 1 for the wave slots 4..7)
        if (theirs + (wid >> 2) > at) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
#elif RS_K7_PRIO == 3
        const int bit = (int)(__builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_s_memtime() >> RS_K7_PRIO_BIT)) & 1) ^ (wid >> 2);
        if (bit) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
#endif
    };
#if RS_K7_PRIO == 4
    if (wid >= 4) __builtin_amdgcn_s_setprio(1);
#endif
    RS_STAMP_DECL
    for (int trip = 0; trip < trips; ++trip) {
        RS_STAMP(15);                                   // loop overhead / tail of the previous group
        balance(RS_K7_PRIO == 2 ? 2 * trip : trip);
        const int gi_raw = wave_g + trip * n_waves;
        const int gi = gi_raw < groups ? gi_raw : groups - 1;
        const int m = gi * 32 + c;
        const bool valid = gi_raw < groups && m < M;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the group's rows and scalars have landed in xraw / xsc
#if defined(RS_K7_ALIGN) && RS_K7_ALIGN >= 1
        __builtin_amdgcn_s_barrier();                               // A/B: start every group in step (VALU phases of the two waves of a SIMD co-issue)
#endif
        const float wi = valid ? xsc[128 + c] : 0.0f;
        const int s_act = reinterpret_cast<const int*>(xsc)[2 * c];
        const float s_adv = xsc[64 + c], s_lpo = xsc[96 + c], s_ret = xsc[160 + c];
        // layer-1 B operands: lane (c, h) feeds input 2s + h of sample c at k-step s; input 11 is the constant 1 (bias column)
        float xv[6];
#pragma unroll
        for (int s6 = 0; s6 < 6; ++s6) xv[s6] = xraw[c * RS_IN + 2 * s6 + h];
        if (h) xv[5] = 1.0f;
        RS_STAMP(0);                                    // wait for the rows, operand reads
        // ---------------- forward ----------------
        f32x16 H1[2], H2[2];
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) H1[it][r] = 0.0f;
        {
            float a0 = w1b[(0 * 6 + 0) * 64 + lane], a1 = w1b[(1 * 6 + 0) * 64 + lane];
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const float b = xv[s];
                float n0 = 0.f, n1 = 0.f;
                if (s + 1 < 6) { n0 = w1b[(0 * 6 + s + 1) * 64 + lane]; n1 = w1b[(1 * 6 + s + 1) * 64 + lane]; }
                H1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, H1[0], 0, 0, 0);
                H1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, H1[1], 0, 0, 0);
                a0 = n0; a1 = n1;
            }
        }
        RS_STAMP(1);                                    // layer 1 MFMAs
#pragma unroll
        for (int it = 0; it < 2; ++it)
            rs_tanh_scaled16(H1[it]);
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // units rs_kappa(4q .. 4q+3, h) = 8q + 4h + 0..3 are consecutive: one b128 read
                const float4 b = *reinterpret_cast<const float4*>(W.b2 + 32 * it + 8 * q + 4 * h);
                H2[it][4 * q + 0] = b.x; H2[it][4 * q + 1] = b.y; H2[it][4 * q + 2] = b.z; H2[it][4 * q + 3] = b.w;
            }
        RS_STAMP(2);                                    // tanh 1 + bias loads
        {
            // both output tiles advance together: two independent accumulators per fragment pair
            const float4* wq = reinterpret_cast<const float4*>(W.w2f) + lane;       // [(it * 2 + kt) * 4 + r4][64 lanes]
            float4 a0 = wq[0], a1 = wq[(1 * 2 + 0) * 4 * 64];
#pragma unroll
            for (int g4 = 0; g4 < 8; ++g4) {
                const int kt = g4 >> 2, r0 = 4 * (g4 & 3);
                float4 n0 = a0, n1 = a1;
                if (g4 + 1 < 8) {
                    n0 = wq[((0 * 2 + ((g4 + 1) >> 2)) * 4 + ((g4 + 1) & 3)) * 64];
                    n1 = wq[((1 * 2 + ((g4 + 1) >> 2)) * 4 + ((g4 + 1) & 3)) * 64];
                }
                H2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, H1[kt][r0 + 0], H2[0], 0, 0, 0);
                H2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, H1[kt][r0 + 0], H2[1], 0, 0, 0);
                H2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, H1[kt][r0 + 1], H2[0], 0, 0, 0);
                H2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, H1[kt][r0 + 1], H2[1], 0, 0, 0);
                H2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, H1[kt][r0 + 2], H2[0], 0, 0, 0);
                H2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, H1[kt][r0 + 2], H2[1], 0, 0, 0);
                H2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, H1[kt][r0 + 3], H2[0], 0, 0, 0);
                H2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, H1[kt][r0 + 3], H2[1], 0, 0, 0);
                a0 = n0; a1 = n1;
            }
        }
        // h1 has fed its last MFMA: its transpose goes to Qt now (B operand of dW2 later, and the source of the tanh'
        // factor of dpre1), so the 32 registers are free for the rest of the group
        rs_stage32(Qt, H1[0], c, h);
        rs_stage32(Qt + 32 * RS_T2, H1[1], c, h);
        RS_STAMP(3);                                    // layer 2 MFMAs + h1^T staging
#if defined(RS_K7_ALIGN) && RS_K7_ALIGN >= 2
        __builtin_amdgcn_s_barrier();
#endif
#pragma unroll
        for (int it = 0; it < 2; ++it)
            rs_tanh_scaled16(H2[it]);
        RS_STAMP(4);                                    // tanh 2
        // output layer: out[o] = sum over the 32 units this lane holds of W3[o][unit] * h2[unit] (one fmaf chain per output, ascending
        // unit, from 0.0f), halves added across lane pairs.  Critic: on the VALU.  Actor: the same chains on the matrix pipe.
        float out[NOUT];
        if constexpr (NOUT == 1) {
            // one output: a single ascending-unit fmaf chain over the register-held weights, no prefetch rotation
            float pacc = 0.0f;
#pragma unroll
            for (int q = 0; q < 32; ++q) pacc = fmaf(w3v[q], H2[q >> 4][q & 15], pacc);
            const float q = rs_other_half(pacc, h);
            out[0] = (h ? (q + pacc) : (pacc + q)) + W.b3[0];
        } else {
            // Eight outputs: two chains of 32 v_mfma_f32_4x4x1_16b_f32, outputs 0..3 and 4..7.  K = 1, so a chain onto one accumulator
            // is the ascending-unit fmaf chain from 0.0f in instruction order, subnormals kept.  Block b of an instruction is the outer
            // product of A lanes 4b..4b+3 and B lanes 4b..4b+3, D[i][j] in register i of lane 4b + j; blocks 0..7 are the h = 0 lanes,
            // 8..15 the h = 1 lanes.  B: the lane's own H2[kt][r]; A: lane l supplies W3[4 set + (l & 3)][32 kt + kappa(r, l >> 5)].
            // Register i of chain `set` is then the partial logit of output 4 set + i over this lane's half of its own sample.
            // The two chains alternate, each filling the other's wait states.
            f32x4 pacc[2];
#pragma unroll
            for (int r = 0; r < 4; ++r) { pacc[0][r] = 0.0f; pacc[1][r] = 0.0f; }
            const float4* wrow = reinterpret_cast<const float4*>(W.w3h) + 8 * h + (lane & 3);     // [8 b][2 h][8 o] float4
            float4 wv[8][2];
#pragma unroll
            for (int b = 0; b < 8; ++b) { wv[b][0] = wrow[16 * b]; wv[b][1] = wrow[16 * b + 4]; }
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int kt = b >> 2, r4 = b & 3;
                pacc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][0].x, H2[kt][4 * r4 + 0], pacc[0], 0, 0, 0);
                pacc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][1].x, H2[kt][4 * r4 + 0], pacc[1], 0, 0, 0);
                pacc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][0].y, H2[kt][4 * r4 + 1], pacc[0], 0, 0, 0);
                pacc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][1].y, H2[kt][4 * r4 + 1], pacc[1], 0, 0, 0);
                pacc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][0].z, H2[kt][4 * r4 + 2], pacc[0], 0, 0, 0);
                pacc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][1].z, H2[kt][4 * r4 + 2], pacc[1], 0, 0, 0);
                pacc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][0].w, H2[kt][4 * r4 + 3], pacc[0], 0, 0, 0);
                pacc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[b][1].w, H2[kt][4 * r4 + 3], pacc[1], 0, 0, 0);
            }
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
                // fixed summation order in both lanes: (half 0) + (half 1); the other half's value by one v_permlane32_swap
                const float p = pacc[o >> 2][o & 3];
                const float q = rs_other_half(p, h);
                out[o] = (h ? (q + p) : (p + q)) + W.b3[o];
            }
        }
        RS_STAMP(5);                                    // output layer (critic: VALU, actor: 2 x 32 4x4x1 MFMAs)
        // ---------------- per-sample loss derivative (identical in both lanes of a sample) ----------------
        float dz[NOUT], sq[4];
        if (NOUT == 8) {
            const int a = s_act;
            const float adv = s_adv, lpo = s_lpo;
            float mx = out[0];
#pragma unroll
            for (int j = 1; j < NOUT; ++j) mx = fmaxf(mx, out[j]);
            float se = 0.f;
#pragma unroll
            for (int j = 0; j < NOUT; ++j) se += __expf(out[j] - mx);
            const float lse = __logf(se);
            float lp[NOUT], pj[NOUT], ent = 0.f, logp = 0.f;
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                lp[j] = (out[j] - mx) - lse;
                pj[j] = __expf(lp[j]);
                ent -= pj[j] * lp[j];
                logp = (a == j) ? lp[j] : logp;
            }
            const float ratio = __expf(logp - lpo);
            const float lo = 1.0f - B.clip_ratio, hi = 1.0f + B.clip_ratio;
            const float clipped = fminf(fmaxf(ratio, lo), hi);
            const float s1 = ratio * adv, s2 = clipped * adv;
            const float surr = fminf(s1, s2);
            const bool inside = ratio >= lo && ratio <= hi;
            const float dr = (inside || s1 < s2) ? adv : 0.0f;
            const float g_lp = -wi * dr * ratio;
            // the entropy bonus is a detached scalar in the reference (`ent = pi.entropy().detach().mean().item()`,
            // ppo.py:1216): alpha * H moves the loss VALUE only, no gradient flows through it
#pragma unroll
            for (int j = 0; j < NOUT; ++j) dz[j] = g_lp * (((a == j) ? 1.0f : 0.0f) - pj[j]);
            sq[0] = wi * (lpo - logp);
            sq[1] = wi * ent;
            sq[2] = wi * ((ratio > hi || ratio < lo) ? 1.0f : 0.0f);
            sq[3] = wi * surr;
        } else {
            const float diff = out[0] - s_ret;
            dz[0] = 2.0f * B.vf_coef * wi * diff;
            sq[0] = wi * diff * diff; sq[1] = 0.f; sq[2] = 0.f; sq[3] = 0.f;
        }
        RS_STAMP(6);                                    // loss derivative
#if RS_K7_PRIO == 2
        balance(2 * trip + 1);
#endif

        // ---------------- backward ----------------
        // the dW3 operands borrow the row landing zone (its rows were consumed by layer 1; the next group's DMA is issued after dW3)
        if constexpr (NOUT == 1) {
            // One output row: dW3[unit] += sum_n dz[n] h2[unit][n], db3 += sum_n dz[n] and the value-loss sum as 2 x 32
            // v_mfma_f32_4x4x1_16b_f32 (K = 1: one instruction per sample, so instruction order is the chain order n = 0..31 the
            // 16x16x4 tiles had).  Block b of an instruction is the outer product of A lanes 4b..4b+3 and B lanes 4b..4b+3, D[i][j] in
            // register i of lane 4b + j.  A: even lanes dz[n], odd lanes the loss term; B: lane l < 32 h2[unit 32 hf + l][n], lanes
            // 32..63 the constant 1.  Register 0 of lane l < 32 is then dW3 of unit 32 hf + l, registers 0 / 1 of the upper lanes are
            // db3 / the loss sum (first half only; what the other registers and the second half's upper lanes collect is never read).
            // h2^T is staged with a row stride of 36 floats so that a lane's 32 samples are eight aligned b128 reads; the tile's last
            // 96 floats, the two A rows and the row of ones lie in the row landing zone, which is free until the DMA issue below.
            constexpr int T4 = 36;
            float* zrow = xraw + 96;                     // [2][32]: dz, loss terms
            float* ones = xraw + 160;                    // [32]
            zrow[32 * h + c] = h ? sq[0] : dz[0];
            ones[c] = 1.0f;
            float4 av[8];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                rs_wave_sync();                          // the previous readers of Pt are done
#pragma unroll
                for (int r = 0; r < 16; ++r) Pt[rs_kappa(r, h) * T4 + c] = H2[hf][r];
                rs_wave_sync();
                if (hf == 0) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) av[q] = *reinterpret_cast<const float4*>(zrow + 32 * (lane & 1) + 4 * q);
                }
                const float* brow = (hf == 0 && h) ? ones : Pt + c * T4;
                float4 bv[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) bv[q] = *reinterpret_cast<const float4*>(brow + 4 * q);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].x, bv[q].x, acc3[hf], 0, 0, 0);
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].y, bv[q].y, acc3[hf], 0, 0, 0);
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].z, bv[q].z, acc3[hf], 0, 0, 0);
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].w, bv[q].w, acc3[hf], 0, 0, 0);
                }
            }
        } else {
            // Eight output rows: dW3[o][unit] += sum_n dz[o][n] h2[unit][n] as two chains of 32 4x4x1 MFMAs, one per 32-unit half hf
            // (K = 1: instruction order is the chain order n = 0..31 the 16x16x4 tiles had).  Lane l = 4b + j supplies
            // A = dz[4 (b & 1) + j][n] = row l & 7 and B = h2[32 hf + 4 (b >> 1) + j][n], so register i of acc3[hf] in lane l is
            // dW3[4 (b & 1) + i][32 hf + 4 (b >> 1) + j]: the 16 blocks are 2 output sets x 8 unit quads, no block is idle.
            // db3 and the four statistics sums are ONE more chain of 32 onto accs with B = 1: lanes 0..11 supply rows 0..11 (dz, then
            // the statistics terms), so register i of lanes 0 / 4 / 8 sums row i / 4 + i / 8 + i (what the lanes from 12 up
            // collect is never read).  Its first 16 instructions sit between the first half's, its last 16 between the second
            // half's, in ascending n: each chain fills the other's wait states.
            // h2^T is staged one half at a time with a row stride of 36 floats and runs 96 floats into the row landing zone, as in
            // the critic; the twelve A rows follow it, [12][36], and run on into xsc, whose scalars have been in registers since the
            // top of the trip.  Both zones are free until the DMA issue below.  Every operand is an aligned ds_read_b128 of four
            // samples; stride 36 puts the rows a 16-lane group reads into different banks.  Both lanes of a sample hold the same
            // dz / sq, so both write all twelve rows: no branch on h.
            constexpr int T4 = 36;
            float* Az = xraw + 96;                       // [12][36]
            static_assert(32 * T4 == 32 * RS_T2 + 96 && 96 + 12 * T4 <= RS_XRAW + RS_XSC, "h2^T tile and A rows end inside xraw + xsc");
#pragma unroll
            for (int o = 0; o < NOUT; ++o) Az[o * T4 + c] = dz[o];
#pragma unroll
            for (int q = 0; q < 4; ++q) Az[(8 + q) * T4 + c] = sq[q];
            const float* arow = Az + (lane & 7) * T4;
            const float* srow = Az + min(l15, 11) * T4;
            const float* brow = Pt + (4 * (lane >> 3) + (lane & 3)) * T4;
            float4 av[8];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                rs_wave_sync();                          // the previous readers of Pt are done
#pragma unroll
                for (int r = 0; r < 16; ++r) Pt[rs_kappa(r, h) * T4 + c] = H2[hf][r];
                rs_wave_sync();
                if (hf == 0) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) av[q] = *reinterpret_cast<const float4*>(arow + 4 * q);
                }
                float4 bv[8], zv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) zv[q] = *reinterpret_cast<const float4*>(srow + 16 * hf + 4 * q);
#pragma unroll
                for (int q = 0; q < 8; ++q) bv[q] = *reinterpret_cast<const float4*>(brow + 4 * q);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float z0 = (q & 1) ? zv[q >> 1].z : zv[q >> 1].x, z1 = (q & 1) ? zv[q >> 1].w : zv[q >> 1].y;
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].x, bv[q].x, acc3[hf], 0, 0, 0);
                    accs = __builtin_amdgcn_mfma_f32_4x4x1f32(z0, 1.0f, accs, 0, 0, 0);
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].y, bv[q].y, acc3[hf], 0, 0, 0);
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].z, bv[q].z, acc3[hf], 0, 0, 0);
                    accs = __builtin_amdgcn_mfma_f32_4x4x1f32(z1, 1.0f, accs, 0, 0, 0);
                    acc3[hf] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[q].w, bv[q].w, acc3[hf], 0, 0, 0);
                }
            }
        }
        RS_STAMP(7);                                    // dW3
        // dh2 = W3^T dz, dpre2 = dh2 * (1 - h2^2) in place of H2
        if (NOUT == 8) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float b = h ? dz[(2 * s + 1) % NOUT] : dz[(2 * s) % NOUT];
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(w3tf[(it * 4 + s) * 64 + lane], b, t, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const rs_f2 d = rs_dtanh2((rs_f2){t[r], t[r + 1]}, (rs_f2){H2[it][r], H2[it][r + 1]});
                    H2[it][r] = d.x; H2[it][r + 1] = d.y;
                }
            }
        } else {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const rs_f2 d = (rs_f2){w3v[kt * 16 + r], w3v[kt * 16 + r + 1]} * (rs_f2){dz[0], dz[0]};
                    const rs_f2 e = rs_dtanh2(d, (rs_f2){H2[kt][r], H2[kt][r + 1]});
                    H2[kt][r] = e.x; H2[kt][r + 1] = e.y;
                }
        }
        // the landing zones are free again: fetch the NEXT group's rows and scalars behind the rest of this group
        {
            const int gn_raw = wave_g + (trip + 1) * n_waves;
            const int gn = gn_raw < groups ? gn_raw : groups - 1;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // every ds_read of the dW3 operands / xsc has returned
            dma_rows(gn);
            dma_scal(gn);
        }
        RS_STAMP(8);                                    // dh2 -> dpre2, DMA issue
#if defined(RS_K7_ALIGN) && RS_K7_ALIGN >= 3
        __builtin_amdgcn_s_barrier();
#endif
        // R3: dh1 = W2^T dpre2 (register operands)  ||  dpre2[0]^T -> Pt
        rs_wave_sync();
        rs_stage32(Pt, H2[0], c, h);
        f32x16 D1[2];
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) D1[it][r] = 0.f;
        {
            const float4* wq = reinterpret_cast<const float4*>(w2tf) + lane;
            float4 a0 = wq[0], a1 = wq[(1 * 2 + 0) * 4 * 64];
#pragma unroll
            for (int g4 = 0; g4 < 8; ++g4) {
                const int kt = g4 >> 2, r0 = 4 * (g4 & 3);
                float4 n0 = a0, n1 = a1;
                if (g4 + 1 < 8) {
                    n0 = wq[((0 * 2 + ((g4 + 1) >> 2)) * 4 + ((g4 + 1) & 3)) * 64];
                    n1 = wq[((1 * 2 + ((g4 + 1) >> 2)) * 4 + ((g4 + 1) & 3)) * 64];
                }
                D1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, H2[kt][r0 + 0], D1[0], 0, 0, 0);
                D1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, H2[kt][r0 + 0], D1[1], 0, 0, 0);
                D1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, H2[kt][r0 + 1], D1[0], 0, 0, 0);
                D1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, H2[kt][r0 + 1], D1[1], 0, 0, 0);
                D1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, H2[kt][r0 + 2], D1[0], 0, 0, 0);
                D1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, H2[kt][r0 + 2], D1[1], 0, 0, 0);
                D1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, H2[kt][r0 + 3], D1[0], 0, 0, 0);
                D1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, H2[kt][r0 + 3], D1[1], 0, 0, 0);
                a0 = n0; a1 = n1;
            }
        }
        // R6's B operand: x[sample 4s + l4][input l15] (input 11 := 1 -> column 11 of dW1 is db1), re-read from L2 (the DMA
        // touched the same lines one group ago); issued here, consumed after dW2
        float xb[8];
        {
            int gi_late = gi;
            asm volatile("" : "+v"(gi_late));           // opaque: keeps the eight loads from being hoisted to the top of the group
#pragma unroll
            for (int s8 = 0; s8 < 8; ++s8) {
                int n = gi_late * 32 + 4 * s8 + l4;
                n = n < M ? n : M - 1;
                xb[s8] = (l15 < RS_IN) ? B.x[(size_t)n * RS_IN + l15] : ((l15 == RS_IN) ? 1.0f : 0.0f);
            }
        }
        // dpre1 = dh1 * (1 - h1^2): h1 comes back from its transposed tile in accumulator layout (conflict-free column reads)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const rs_f2 hv = {Qt[(32 * it + rs_kappa(r, h)) * RS_T2 + c], Qt[(32 * it + rs_kappa(r + 1, h)) * RS_T2 + c]};
                const rs_f2 d = rs_dtanh2((rs_f2){D1[it][r], D1[it][r + 1]}, hv);
                D1[it][r] = d.x; D1[it][r + 1] = d.y;
            }
        rs_wave_sync();
        RS_STAMP(9);                                    // R3 dh1 MFMAs + dpre2^T staging + dpre1
        // R4 / R5: dW2[it][kt] += dpre2[it] . h1^T (16 k-steps over the 32 samples); db2 row sums from the staged tile
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            if (it == 1) {
                rs_wave_sync();
                rs_stage32(Pt, H2[1], c, h);
                rs_wave_sync();
            }
            float a_c = Pt[c * RS_T2 + h], b0_c = Qt[c * RS_T2 + h], b1_c = Qt[(32 + c) * RS_T2 + h];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                float a_n = 0.f, b0_n = 0.f, b1_n = 0.f;
                if (s + 1 < 16) {
                    a_n = Pt[c * RS_T2 + 2 * (s + 1) + h];
                    b0_n = Qt[c * RS_T2 + 2 * (s + 1) + h];
                    b1_n = Qt[(32 + c) * RS_T2 + 2 * (s + 1) + h];
                }
                acc2[it][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c, b0_c, acc2[it][0], 0, 0, 0);
                acc2[it][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c, b1_c, acc2[it][1], 0, 0, 0);
                a_c = a_n; b0_c = b0_n; b1_c = b1_n;
            }
            // db2[32it + c] += sum over the 32 samples of dpre2: lane (c, h) sums samples 16h .. 16h+15 of row c
            float rs = 0.0f;
#pragma unroll
            for (int n = 0; n < 16; ++n) rs += Pt[c * RS_T2 + 16 * h + n];
            rs += rs_other_half(rs, h);
            if constexpr (NOUT == 1) db2r[it] += rs;    // same adds in the same order, handed to the epilogue in registers
            else if (h == 0) dbl[32 * it + c] += rs;
        }
        RS_STAMP(10);                                   // R4 / R5 dW2 + db2
        // R6: dW1[unit][input] += sum_n dpre1[unit][n] x[input][n]  (16x16x4, 8 k-steps per half)
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            rs_wave_sync();
            rs_stage32(Pt, D1[it], c, h);
            rs_wave_sync();
            float a0_c = Pt[l15 * RS_T2 + l4], a1_c = Pt[(16 + l15) * RS_T2 + l4];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                float a0_n = 0.f, a1_n = 0.f;
                if (s + 1 < 8) {
                    a0_n = Pt[l15 * RS_T2 + 4 * (s + 1) + l4];
                    a1_n = Pt[(16 + l15) * RS_T2 + 4 * (s + 1) + l4];
                }
                acc1[2 * it + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0_c, xb[s], acc1[2 * it + 0], 0, 0, 0);
                acc1[2 * it + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1_c, xb[s], acc1[2 * it + 1], 0, 0, 0);
                a0_c = a0_n; a1_c = a1_n;
            }
        }
        rs_wave_sync();
        RS_STAMP(11);                                   // R6 dW1
    }
    // ---- one partial slab per WORKGROUP, parameter order {w1, b1, w2, b2, w3, b3}.  Every wave writes its accumulators to a
    // slab of its own in LDS, then all 512 threads add the eight slabs in wave order, (((0 + w0) + w1) + ...) + w7 (fixed order ->
    // reproducible), and write the sums straight to the workgroup's slab in HBM.  Eight private slabs do not fit the LDS at
    // once; the weight fragments are dead by now, so the whole allocation is reused in two rounds: dW2 (8 x 4096 floats), then
    // everything else (8 x RS_REST floats) and the float64 statistics.
    constexpr int RS_REST = rs_net_params(NOUT) - 64 * 64;          // w1, b1, b2, w3, b3
    static_assert(8 * 64 * 64 <= rs_grad2_lds_floats(NOUT) && 8 * ((RS_REST + 1) & ~1) + 2 * 8 * 5 <= rs_grad2_lds_floats(NOUT),
                  "the epilogue's slabs must fit K7's LDS");
    // thread and lane indices afresh, opaque to the compiler: derived from the ones above, the epilogue's addresses and loop bounds
    // are computed in front of the trip loop and held across it, in a kernel that has no register to spare (they went to scratch)
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int lane_e = tid_e & 63, h_e = lane_e >> 5, c_e = lane_e & 31, l15_e = lane_e & 15, l4_e = lane_e >> 4;
#if RS_K7_PRIO != 0
    __builtin_amdgcn_s_setprio(0);                    // the epilogue runs at equal priority
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last trip's look-ahead DMA has landed: nothing writes LDS behind our back
    // (dbl lives in the region being overwritten: read it first); the critic's sums are in registers, unit 32 it + c in lane (c, it)
    const float db2v = NOUT == 1 ? (h_e ? db2r[1] : db2r[0]) : dbl[lane_e];
    RS_SKEW_LOOP_END(sk_slots)
    __syncthreads();                                  // every wave is done with its staging tiles and the fragments
    RS_SKEW_RELEASED
    RS_SKEW_PAIRS(NOUT == 8 ? 0 : 1, sk_slots)
    float* outp = partial + (size_t)bid * rs_net_params(NOUT);
    {
        float* g_w2 = smem_f + wid * (64 * 64);
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * it + rs_kappa(r, h_e);
                g_w2[row * 64 + c_e] = acc2[it][0][r];
                g_w2[row * 64 + 32 + c_e] = acc2[it][1][r];
            }
    }
    __syncthreads();
    for (int i = tid_e; i < 64 * 64; i += blockDim.x) {
        float v = 0.0f + smem_f[i];
#pragma unroll
        for (int wv = 1; wv < 8; ++wv) v += smem_f[wv * (64 * 64) + i];
        outp[64 * RS_IN + 64 + i] = v;
    }
    // The actor's accs (4x4x1 blocks 0..2, every column identical): rows 0..NOUT-1 = db3, rows 8..11 = statistics sums of this
    // wave; bring them to lane 0 (row r lives in lane 4 (r / 4), register r % 4)
    // The critic's 4x4x1 accumulators: acc3[hf][0] of lane l < 32 = dW3 of unit 32 hf + l, acc3[0][0] / acc3[0][1] of the upper lanes
    // = db3 / the value-loss sum.
    float db3r[NOUT];
    double sv[5];
    if constexpr (NOUT == 1) {
        db3r[0] = __shfl(acc3[0][0], 32);
        sv[0] = 0.0; sv[1] = 0.0; sv[2] = 0.0; sv[3] = (double)__shfl(acc3[0][1], 32); sv[4] = 0.0;
    } else {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) db3r[o] = __shfl(accs[o & 3], 4 * (o >> 2));
        const float t0 = __shfl(accs[0], 8), t1 = __shfl(accs[1], 8), t2 = __shfl(accs[2], 8), t3 = __shfl(accs[3], 8);
        sv[0] = (double)t0; sv[1] = (double)t1; sv[2] = (double)t2; sv[3] = 0.0; sv[4] = (double)t3;
    }
    constexpr int RS_RSTR = (RS_REST + 1) & ~1;       // slab stride of round two (even: the doubles behind the slabs stay aligned)
    double* sred = reinterpret_cast<double*>(smem_f + 8 * RS_RSTR);     // [8 waves][5]
    __syncthreads();                                  // round one has been read
    {
        float* g_w1 = smem_f + wid * RS_RSTR, *g_b1 = g_w1 + 64 * RS_IN, *g_b2 = g_b1 + 64, *g_w3 = g_b2 + 64, *g_b3 = g_w3 + NOUT * 64;
        g_b2[lane_e] = db2v;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * u + 4 * l4_e + q;
                if (l15_e < RS_IN) g_w1[row * RS_IN + l15_e] = acc1[u][q];
                if (l15_e == RS_IN) g_b1[row] = acc1[u][q];
            }
        if constexpr (NOUT == 8) {
            // register i of acc3[hf] in lane 4b + j = dW3[4 (b & 1) + i][32 hf + 4 (b >> 1) + j]
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    g_w3[(4 * ((lane_e >> 2) & 1) + i) * 64 + 32 * hf + 4 * (lane_e >> 3) + (lane_e & 3)] = acc3[hf][i];
        }
        if (NOUT == 1 && lane_e < 32) { g_w3[lane_e] = acc3[0][0]; g_w3[32 + lane_e] = acc3[1][0]; }
        if (lane_e == 0) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o) g_b3[o] = db3r[o];
#pragma unroll
            for (int q = 0; q < 5; ++q) sred[wid * 5 + q] = sv[q];
        }
    }
    __syncthreads();
    for (int i = tid_e; i < RS_REST; i += blockDim.x) {
        float v = 0.0f + smem_f[i];
#pragma unroll
        for (int wv = 1; wv < 8; ++wv) v += smem_f[wv * RS_RSTR + i];
        outp[i < 64 * RS_IN + 64 ? i : i + 64 * 64] = v;          // {w1, b1} lie in front of w2 in the slab, {b2, w3, b3} behind it
    }
    if (tid_e < 5) {
        double v = 0.0 + sred[tid_e];
#pragma unroll
        for (int wv = 1; wv < 8; ++wv) v += sred[wv * 5 + tid_e];
        stat_partial[(size_t)bid * 5 + tid_e] = v;
    }
    RS_STAMP_EXIT(NOUT == 8 ? 0 : 1);
    RS_SKEW_EXIT(NOUT == 8 ? 0 : 1);
}

template <int NOUT>
__global__ void __launch_bounds__(512, 2) rs_ppo_grad2_kernel(RsMlpParams prm, rs_ppo_batch B, float* __restrict__ partial,
                                                              double* __restrict__ stat_partial, const int* __restrict__ stop,
                                                              const rs_update_state* __restrict__ ust, int* __restrict__ snap) {
    rs_ppo_grad2_body<NOUT>(prm, B, partial, stat_partial, stop, ust, snap, blockIdx.x, gridDim.x);
}

// Both passes of one Adam step in ONE grid of 2G workgroups: 0..G-1 are the actor launch's workgroups, G..2G-1 the critic launch's
// (slab, statistics row, snap copy and early exit exactly as in the two launches, so every bit is the same).  Workgroups are handed
// out in index order and one fits a CU, so a critic workgroup starts on a CU as soon as an actor workgroup retires there: no launch
// gap between the networks, no drain behind the slowest actor workgroup, and the critic's prologue runs next to the actor's tail.
__global__ void __launch_bounds__(512, 2) rs_ppo_grad2_pair_kernel(RsMlpParams pa, RsMlpParams pc, rs_ppo_batch B, float* __restrict__ partial_a,
                                                                   float* __restrict__ partial_c, double* __restrict__ stat_a,
                                                                   double* __restrict__ stat_c, const int* __restrict__ stop,
                                                                   const rs_update_state* __restrict__ ust, int* __restrict__ snap) {
    const int G = gridDim.x >> 1;
    if ((int)blockIdx.x < G) rs_ppo_grad2_body<8>(pa, B, partial_a, stat_a, stop, nullptr, nullptr, blockIdx.x, G);
    else rs_ppo_grad2_body<1>(pc, B, partial_c, stat_c, stop, ust, snap, blockIdx.x - G, G);
}

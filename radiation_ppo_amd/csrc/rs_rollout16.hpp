// rs_rollout16.hpp -- K6: the fused collector with 16 envs per wave.
//
// A wave owns 16 envs: 4096 envs are 256 waves (every CU busy), the MLP runs on v_mfma_f32_16x16x4_f32 tiles (152
// MFMAs of 32 cycles per lock-step), and the env step -- a latency-bound scalar f64 chain whose cost does not depend on
// how many lanes run it -- is paid once per 16 envs.  (A 64-envs-per-wave layout was measured in round 1: 64 waves on 64
// of the 256 CUs and 304 MFMAs of 64 cycles per lock-step on one SIMD: slower.)
//
// Lane mapping: lane l = (j = l&15, g = l>>4).  Env slot j of the wave is env n = 16*block + j; its state and all
// per-env logic live in lane (j, 0).  For the MLP the four lanes (j, 0..3) share sample j:
//   A lane l: W[16it + (l&15)][k = 4s + (l>>4)]     B lane l: In[k = 4s + (l>>4)][sample l&15]
//   D lane l, reg q: sample l&15, unit 16it + 4*(l>>4) + q
// so the k-step (ut, q) of the next layer consumes unit 16ut + 4g + q straight from the accumulator registers
// (the 16x16 analogue of the kappa trick in rs_mlp.hpp).
//
// Two waves per workgroup (round 4).  A lone wave issues one instruction per ~3.4 ns whatever it is (profiles/r04_valu_cost.txt), and
// a lock-step was one serial stream of ~2 900 of them although only  observation -> actor -> draw -> env step -> observation  is a
// dependence chain: the critic's value is stored, never fed back.  Wave 0 walks the chain; wave 1 (another SIMD of the same CU, idle
// before) evaluates the critic on the observations wave 0 leaves in an LDS mailbox -- the pre-reset one for the bootstrap value, the
// post-reset one for the envs that were cut -- and writes val / last_val itself.  One workgroup barrier per lock-step, mailbox double
// buffered (wave 0 runs a step ahead).  With the critic skipped outright the lock-step took 7.6 instead of 9.6 us: that is the bound.
//
// Wave 0's chain itself (round 10): what is constant for the launch or only changes in the wave's own registers does not go through
// memory in every lock-step.  The actor's MFMA operands are read from LDS once (RsMlp16::Regs; the template without obstacles, which
// has the registers), its output layer runs as two 4x4x1 MFMA chains like K7's, and the env state stays in registers between the
// lock-steps (RsEnvRegs / RsAgentRegs, rs_agent_step_core); the env arrays are written and re-read around a reset only.  Buffers,
// env arrays and carried state keep their bits (tests/test_k6_chain_bits_gpu.py).
//
// The draws (round 14).  The env step's measurement was a serial rejection loop that ran until the slowest of the wave's 16 envs had
// accepted (2.1 trips per lock-step) while 48 of wave 0's lanes idled, and the action draw hashed a Philox block of its own once the
// logits were there.  Now one philox4x32_10 call ahead of the forward pass serves both: lane (j, 0) hashes the action uniform's block,
// lanes (j, 1..3) the blocks of candidates 0..2 of the measurement draw, which rs_poisson_group<1> (rs_device.hpp) evaluates side by
// side in the env step; the serial loop is left for an env with three rejections (0.03 trips per lock-step).  For that all four lanes
// of an env run the step core in both templates, with identical values.  Without obstacles the critic's wave also writes the buffer's
// observation rows from the messages it reads.  Same bits (tests/test_k6_poisson_group_gpu.py).
//
// Tile waves (round 15; the template without obstacles).  The actor's two hidden layers were 76 MFMAs and 32 tanh back to back in wave
// 0 although their four output tiles are independent accumulator chains.  The workgroup now has four waves, one per SIMD (at 400
// registers no two share one), and each computes ONE tile: wave 0 tile 0, wave 1 tile 3 (ahead of its critic work), waves 2 and 3
// tiles 1 and 2 (RsMlp16::tile_layer1 / tile_layer2, operands parked per wave).  Waves 1..3 take the observation from the mailbox
// message wave 0 completes before the lock-step's barrier: the post-reset row where flag bit 0 (cut) is set, else the pre-reset row,
// which is what wave 0 goes on with.  Three workgroup barriers per lock-step t, executed by every wave, nothing else is waited on:
//   obs(t - 1)  message t - 1 complete (the barrier there was before; obs(-1) in the prologue)
//   H1(t)       every wave has stored its layer-1 tile to xch1; behind it every wave loads all four
//   H2(t)       waves 1..3 have stored their layer-2 tiles to xch2; behind it wave 0 loads them, runs the output layer and the chain
// Counts: wave 0 executes obs(-1) and then H1, H2, obs in each of its T lock-steps; waves 1..3 loop over t = -1 .. T - 1, execute
// obs(t) and then, if lock-step t + 1 exists, H1(t + 1) and H2(t + 1): 3 T + 1 in every wave for every T >= 1, in the same order.
// The exchange arrays are single-buffered: xch1 is read between H1(t) and H2(t) (a __syncthreads waits for the wave's LDS loads
// before the barrier) and rewritten after obs(t); xch2 is read by wave 0 between H2(t) and obs(t) and rewritten after H1(t + 1).  A
// tile is rewritten only after every reader has passed a later barrier.  The mailbox stays double buffered: wave 1 reads message t
// for the critic while wave 0 writes message t + 1.  The order of every sum is the one of RsMlp16::hidden, so the buffers keep their
// bits (tests/test_k6_tile_waves_gpu.py).  -DRS_K6_TILE_WAVES=2: waves 2 and 3 with two interleaved tiles each; =0: as before.
// A four-wave workgroup has a CU to itself where two two-wave workgroups shared one, so the tile waves pay while there are no more
// workgroups than CUs (4096 envs on 256 CUs: the SIMDs they use were idle).  Beyond that rs_rollout launches rs_rollout16_wide_kernel,
// the same body with two waves; the obstacle template (config 3: 512 workgroups) stays on two waves for the same reason.
#pragma once
#include "rs_mlp.hpp"

__host__ __device__ constexpr int rs_mlp16_lds_floats(int nout) { return 4 * 3 * 64 + 4 * 16 * 64 + 64 + 4 * nout * 16 + nout; }

template <int NOUT>
struct RsMlp16 {
    float* w1f;   // [4 it][3 s][64]   2log2e * W1[16it + (l&15)][4s + (l>>4)], column 11 = 2log2e * b1 (x[11] := 1)
    float* w2f;   // [4 it][16 ks][64] 2log2e * W2[16it + (l&15)][16ut + 4(l>>4) + q], ks = 4ut + q
    float* b2;    // [64] 2log2e * b2
    float* w3g;   // [4 g][NOUT][16]   W3[o][16ut + 4g + q]
    float* b3;    // [NOUT]
    __device__ __forceinline__ void carve(float* base) {
        w1f = base; w2f = w1f + 4 * 3 * 64; b2 = w2f + 4 * 16 * 64; w3g = b2 + 64; b3 = w3g + 4 * NOUT * 16;
    }
    __device__ __forceinline__ void fill(const RsMlpParams& p) {
        const int tid = threadIdx.x, nt = blockDim.x;
        for (int i = tid; i < 4 * 3 * 64; i += nt) {
            const int l = i & 63, s = (i >> 6) % 3, it = i / (3 * 64);
            const int row = 16 * it + (l & 15), k = 4 * s + (l >> 4);
            w1f[i] = RS_TANH_PRESCALE * ((k < RS_IN) ? p.w1[row * RS_IN + k] : p.b1[row]);
        }
        for (int i = tid; i < 4 * 16 * 64; i += nt) {
            const int l = i & 63, ks = (i >> 6) & 15, it = i >> 10;
            const int unit = 16 * (ks >> 2) + 4 * (l >> 4) + (ks & 3);
            w2f[i] = RS_TANH_PRESCALE * p.w2[(16 * it + (l & 15)) * RS_HID + unit];
        }
        for (int i = tid; i < 64; i += nt) b2[i] = RS_TANH_PRESCALE * p.b2[i];
        for (int i = tid; i < 4 * NOUT * 16; i += nt) {
            const int q16 = i & 15, o = (i >> 4) % NOUT, g = i / (16 * NOUT);
            w3g[i] = p.w3[o * RS_HID + 16 * (q16 >> 2) + 4 * g + (q16 & 3)];
        }
        for (int i = tid; i < NOUT; i += nt) b3[i] = p.b3[i];
    }
    // The operands of forward() that belong to this lane, read once: they are constant for a launch.  K6's wave 0 keeps the actor's
    // in registers for all its lock-steps (walls-off / no-obstacle template: 124 of the 512 registers a lone wave of a SIMD may use)
    // instead of reading them from LDS in every lock-step, where each read and its wait is an issue slot of the serial chain.
    struct Regs {
        float w1[4 * 3], w2[4 * 16], b2[4 * 4];
        float w3[2][16];      // NOUT == 8: A operands of the output layer's two 4x4x1 chains, W3[4 set + (l & 3)][16 ut + 4 g + q] at [set][4 ut + q]
    };
    __device__ __forceinline__ void load_w3(float (&w3)[2][16]) const {
        const int lane = threadIdx.x & 63, g = lane >> 4;
#pragma unroll
        for (int set = 0; set < 2; ++set) {
            const float4* w = reinterpret_cast<const float4*>(w3g + (g * NOUT + 4 * set + (lane & 3)) * 16);
#pragma unroll
            for (int ut = 0; ut < 4; ++ut) {
                const float4 wv = w[ut];
                w3[set][4 * ut + 0] = wv.x; w3[set][4 * ut + 1] = wv.y; w3[set][4 * ut + 2] = wv.z; w3[set][4 * ut + 3] = wv.w;
            }
        }
    }
    // The MFMA A operands are parked in accumulation registers, which the matrix instructions read directly: left to itself the
    // register allocator keeps them among the 256 architectural VGPRs, where the env step's float64 chains need the room.
    static __device__ __forceinline__ float park(float v) { float a; asm("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(v)); return a; }
    __device__ __forceinline__ void load(Regs& r) const {
        const int lane = threadIdx.x & 63, g = lane >> 4;
#pragma unroll
        for (int i = 0; i < 4 * 3; ++i) r.w1[i] = park(w1f[i * 64 + lane]);
#pragma unroll
        for (int i = 0; i < 4 * 16; ++i) r.w2[i] = park(w2f[i * 64 + lane]);
#pragma unroll
        for (int i = 0; i < 4 * 4; ++i) r.b2[i] = b2[16 * (i >> 2) + 4 * g + (i & 3)];
        if constexpr (NOUT == 8) {
            load_w3(r.w3);
#pragma unroll
            for (int i = 0; i < 32; ++i) r.w3[i >> 4][i & 15] = park(r.w3[i >> 4][i & 15]);
        }
    }
    // the two hidden layers for the wave's 16 samples; xs[k] = input k of sample (lane&15), already broadcast to the 4 lanes.
    // REG: operands from r (see Regs), else from LDS.
    template <bool REG>
    __device__ __forceinline__ void hidden(const float (&xs)[RS_IN_PAD], f32x4 (&H2)[4], const Regs& r) const {
        const int lane = threadIdx.x & 63, g = lane >> 4;
        f32x4 H1[4];
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int q = 0; q < 4; ++q) { H1[it][q] = 0.0f; H2[it][q] = REG ? r.b2[4 * it + q] : b2[16 * it + 4 * g + q]; }
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const float b = (g == 0) ? xs[4 * s] : (g == 1) ? xs[4 * s + 1] : (g == 2) ? xs[4 * s + 2] : xs[4 * s + 3];
#pragma unroll
            for (int it = 0; it < 4; ++it)
                H1[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(REG ? r.w1[it * 3 + s] : w1f[(it * 3 + s) * 64 + lane], b, H1[it], 0, 0, 0);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int q = 0; q < 4; ++q) H1[it][q] = rs_tanh_scaled(H1[it][q]);
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const float b = H1[ks >> 2][ks & 3];
#pragma unroll
            for (int it = 0; it < 4; ++it)
                H2[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(REG ? r.w2[it * 16 + ks] : w2f[(it * 16 + ks) * 64 + lane], b, H2[it], 0, 0, 0);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int q = 0; q < 4; ++q) H2[it][q] = rs_tanh_scaled(H2[it][q]);
    }
    // The same two layers, NT of the four output tiles per wave (K6's tile waves): the tiles it0 .. it0 + NT - 1 are independent
    // accumulator chains, so a wave that owns them computes what hidden() computes for them, instruction for instruction: layer 1 from
    // 0.0f over s = 0..2, layer 2 from b2 over ks = 0..15, rs_tanh_scaled on the same values.  The operands of its tiles are parked in
    // accumulation registers once per launch, as in Regs (19 per tile).  D of tile ut in lane l is exactly the B operand lane l needs
    // for the k-steps ks = 4 ut + q of the next layer in every wave, so the waves exchange whole accumulators through LDS
    // ([4 tiles][64 lanes] f32x4, one 16-byte store and four 16-byte loads per lane) without moving a value between lanes.
    template <int NT> struct TileRegs { float w1[NT * 3], w2[NT * 16], b2[NT * 4]; };
    template <int NT>
    __device__ __forceinline__ void load_tiles(TileRegs<NT>& r, int it0) const {
        const int lane = threadIdx.x & 63, g = lane >> 4;
#pragma unroll
        for (int i = 0; i < NT * 3; ++i) r.w1[i] = park(w1f[(it0 * 3 + i) * 64 + lane]);
#pragma unroll
        for (int i = 0; i < NT * 16; ++i) r.w2[i] = park(w2f[(it0 * 16 + i) * 64 + lane]);
#pragma unroll
        for (int i = 0; i < NT * 4; ++i) r.b2[i] = b2[16 * (it0 + (i >> 2)) + 4 * g + (i & 3)];
    }
    // b[s] = input 4 s + (lane >> 4) of sample lane & 15
    template <int NT>
    __device__ __forceinline__ void tile_layer1(const float (&b)[3], const TileRegs<NT>& r, f32x4 (&H1)[NT]) const {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) H1[n][q] = 0.0f;
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int n = 0; n < NT; ++n) H1[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(r.w1[n * 3 + s], b[s], H1[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) H1[n][q] = rs_tanh_scaled(H1[n][q]);
    }
    // H1: all four tiles of layer 1 (after the exchange)
    template <int NT>
    __device__ __forceinline__ void tile_layer2(const f32x4 (&H1)[4], const TileRegs<NT>& r, f32x4 (&H2)[NT]) const {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) H2[n][q] = r.b2[4 * n + q];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const float b = H1[ks >> 2][ks & 3];
#pragma unroll
            for (int n = 0; n < NT; ++n) H2[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(r.w2[n * 16 + ks], b, H2[n], 0, 0, 0);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) H2[n][q] = rs_tanh_scaled(H2[n][q]);
    }
    // fixed-order tree over the four lanes of the sample: (g0 + g1) + (g2 + g3) in every lane, then the bias
    __device__ __forceinline__ float combine(float p, int o) const {
        const int g = (threadIdx.x & 63) >> 4;
        const float q1 = __shfl_xor(p, 16);
        const float s01 = (g & 1) ? (q1 + p) : (p + q1);
        const float q2 = __shfl_xor(s01, 32);
        return ((g & 2) ? (q2 + s01) : (s01 + q2)) + b3[o];
    }
    // output layer: out[o] = tree over g of the lane's partial sum p = sum over (ut, q) of W3[o][16 ut + 4 g + q] * H2[ut][q], one
    // fmaf chain per output in the order ut = 0..3, q = 0..3 from 0.0f
    __device__ __forceinline__ void output(const f32x4 (&H2)[4], float (&out)[NOUT]) const {
        const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            const float4* w = reinterpret_cast<const float4*>(w3g + (g * NOUT + o) * 16);
            float p = 0.0f;
#pragma unroll
            for (int ut = 0; ut < 4; ++ut) {
                const float4 wv = w[ut];
                p = fmaf(wv.x, H2[ut][0], p); p = fmaf(wv.y, H2[ut][1], p);
                p = fmaf(wv.z, H2[ut][2], p); p = fmaf(wv.w, H2[ut][3], p);
            }
            out[o] = combine(p, o);
        }
    }
    // The same chains on the matrix pipe (NOUT == 8), as in K7's actor pass (rs_ppo_grad2.hpp): two alternating chains of 16
    // v_mfma_f32_4x4x1_16b_f32, outputs 0..3 and 4..7.  K = 1, so a chain onto one accumulator is the fmaf chain above in
    // instruction order (scripts/micro/mfma4_chain_bits.hip: the same words, subnormals, NaN and -0 included).  Block b of an
    // instruction is the outer product of A lanes 4b..4b+3 and B lanes 4b..4b+3, D[i][j] in register i of lane 4b + j; the four lanes
    // of a block share g.  B: the lane's own H2[ut][q]; A: lane l supplies W3[4 set + (l & 3)][16 ut + 4 g + q] (w3[set][4 ut + q]).
    // Register i of chain `set` is then p of output 4 set + i for this lane's sample.
    __device__ __forceinline__ void output_mfma(const f32x4 (&H2)[4], float (&out)[NOUT], const float (&w3)[2][16]) const {
        static_assert(NOUT == 8, "two chains of four outputs");
        f32x4 pacc[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) { pacc[0][i] = 0.0f; pacc[1][i] = 0.0f; }
#pragma unroll
        for (int ut = 0; ut < 4; ++ut)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                pacc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(w3[0][4 * ut + q], H2[ut][q], pacc[0], 0, 0, 0);
                pacc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(w3[1][4 * ut + q], H2[ut][q], pacc[1], 0, 0, 0);
            }
#pragma unroll
        for (int o = 0; o < NOUT; ++o) out[o] = combine(pacc[o >> 2][o & 3], o);
    }
    __device__ __forceinline__ void forward(const float (&xs)[RS_IN_PAD], float (&out)[NOUT]) const {
        f32x4 H2[4];
        Regs none;
        hidden<false>(xs, H2, none);
        output(H2, out);
    }
};

// broadcast the inputs of sample j (held by lane (j, 0)) to its four lanes
__device__ __forceinline__ void rs_bcast_x16(const float (&xo)[RS_IN_PAD], float (&xs)[RS_IN_PAD]) {
    const int src = threadIdx.x & 15;
#pragma unroll
    for (int k = 0; k < RS_IN_PAD; ++k) xs[k] = __shfl(xo[k], src);
}

constexpr int RS_MB_PRE = 0, RS_MB_POST = 16 * RS_IN_PAD, RS_MB_FLAGS = 2 * 16 * RS_IN_PAD, RS_MB_SLOT = 2 * 16 * RS_IN_PAD + 16;   // words
__host__ __device__ constexpr int rs_rollout16_mailbox_bytes() { return 2 * RS_MB_SLOT * 4; }

// What wave 0 keeps out of its lock-step chain (RS_K6_PARENT_CHAIN: A/B switch, the chain as it was before).  The obstacle template
// sits at the register limit already; it takes what adds no spill.
#ifdef RS_K6_PARENT_CHAIN
constexpr bool RS_K6_SHORT = false;
#else
constexpr bool RS_K6_SHORT = true;
#endif
// A/B switches of round 14 (profiles/r14_k6_poisson_ab.txt).  RS_K6_SERIAL_DRAW: the serial rs_poisson, the action draw's own Philox call
// inside the softmax and the observation rows from wave 0, as before; -DRS_K6_OBS_BY_WAVE1=false: the observation rows alone as before.
#ifdef RS_K6_SERIAL_DRAW
constexpr bool RS_K6_GROUP = false;
#else
constexpr bool RS_K6_GROUP = true;
#endif
#ifndef RS_K6_OBS_BY_WAVE1
#define RS_K6_OBS_BY_WAVE1 true
#endif
// A/B switch of round 15 (profiles/r15_k6_tile_waves_ab.txt): how many waves share the actor's hidden layers.  4: one output tile per
// wave of a four-wave workgroup; 2: waves 2 and 3 with two interleaved tiles each, wave 0 only waits; 0: all four tiles in wave 0 of a
// two-wave workgroup, as before.
#ifndef RS_K6_TILE_WAVES
#define RS_K6_TILE_WAVES 4
#endif
static_assert(RS_K6_TILE_WAVES == 0 || RS_K6_TILE_WAVES == 2 || RS_K6_TILE_WAVES == 4, "RS_K6_TILE_WAVES: 0, 2 or 4");
#ifndef RS_K6_TILE_WAVES_OBS                 // the same for the obstacle template, which is left as it was
#define RS_K6_TILE_WAVES_OBS 0
#endif
static_assert(RS_K6_TILE_WAVES_OBS == 0 || RS_K6_TILE_WAVES_OBS == 2 || RS_K6_TILE_WAVES_OBS == 4, "RS_K6_TILE_WAVES_OBS: 0, 2 or 4");
template <bool HAS_OBS> constexpr int rs_k6_tile_waves = (RS_K6_SHORT && RS_K6_GROUP && RS_K6_OBS_BY_WAVE1) ? (HAS_OBS ? RS_K6_TILE_WAVES_OBS : RS_K6_TILE_WAVES) : 0;
// TW: the tile waves of the kernel body; rs_rollout16_kernel<HAS_OBS> has the default, rs_rollout16_wide_kernel none
template <bool HAS_OBS, int TW = rs_k6_tile_waves<HAS_OBS>> struct RsK6Cfg {
    // the actor's hidden layers on tile waves (0: none), see "Tile waves" in the header.  Not with obstacles: a four-wave workgroup has a
    // CU to itself, and config 3's 512 workgroups (8192 envs) then run in two rounds: its collect took 30.4 ms instead of 16.7
    static constexpr int tile_waves = TW;
    static constexpr int tiles_per_wave = tile_waves ? 4 / tile_waves : 4;
    static constexpr int waves = tile_waves ? 4 : 2;                 // of the workgroup (each on a SIMD of its own: the registers allow no two)
    static constexpr bool reg_weights = RS_K6_SHORT && !HAS_OBS;     // actor operands in registers for the launch (RsMlp16::Regs)
    static constexpr bool mfma_out = RS_K6_SHORT;                    // actor output layer on 4x4x1 MFMA chains
    static constexpr bool reg_state = RS_K6_SHORT;                   // env state in registers across the lock-steps (RsEnvRegs / RsAgentRegs)
    // one Philox call per lock-step, ahead of the forward pass: lane group 0 hashes the action uniform's block, groups 1..3 the
    // candidates 0..2 of the measurement draw, which rs_poisson_group<1> then evaluates side by side
    static constexpr bool group_draw = RS_K6_GROUP && reg_state;
    // the buffer's observation row t + 1 is the row of message t (the post-reset one where the env was cut): the critic's wave, which
    // reads the message anyway and is off the chain, writes it; wave 0's eleven tile stores and its copy-out loop go.  Not with
    // obstacles: that template then spills 270 registers instead of 18.
    static constexpr bool obs_by_wave1 = RS_K6_SHORT && RS_K6_GROUP && RS_K6_OBS_BY_WAVE1 && !HAS_OBS;
};

// the two exchange arrays of the tile waves, [4 tiles][64 lanes] f32x4 each, behind the mailbox (whose size keeps them 16-byte aligned)
template <bool HAS_OBS> __host__ __device__ constexpr int rs_rollout16_exchange_bytes() { return RsK6Cfg<HAS_OBS>::tile_waves ? 2 * 4 * 64 * 16 : 0; }
static_assert(rs_rollout16_mailbox_bytes() % 16 == 0 && (RS_WAVE * RS_OBS_DIM * 4 + RS_WAVE * 4 + 2 * RS_WAVE) % 16 == 0, "exchange arrays: 16-byte aligned");

// Diagnostic build only (-DRS_K6_STAMPS, scripts/k6_stamps.py): s_memtime stamps at the phase boundaries of wave 0's lock-step,
// summed per wave in scalar registers and added (lane 0, plain vector atomics) to a table no other code reads.  Slot 14 holds the
// launch's 100 MHz ticks, slot 15 the lock-steps counted.  Slots 8..12 look into the draws: 8 the cycles of the measurement draw inside
// "env step", 9 the trips rs_poisson's serial loop needs per lock-step (the candidates of the wave's slowest env), summed, 10 the same
// beyond three (the serial trips the grouped sampler has left), 11 the cycles spent counting them (inside "env step": the script takes
// them out), 12 the cycles of the Philox call of the action draw (group_draw: of the lock-step's one call).  The product build
// contains none of it.  Slot 13 is a phase of its own: that one call ("draw blocks"), kept out of "hidden layers".  Slots 16 and 17
// belong to "hidden layers" with tile waves: wave 0's cycles from its H1 (H2) tile store to the last tile of the exchange read back,
// i.e. the workgroup barrier, the wait for the slowest tile wave, and the 16-byte loads.
#ifdef RS_K6_STAMPS
#define RS_K6_NPH 20
__device__ unsigned long long rs_k6_stamp_table[2][RS_K6_NPH];
__device__ __forceinline__ unsigned long long rs_k6_now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#define RS_K6STAMP_DECL unsigned long long k6_acc[RS_K6_NPH] = {0}; const unsigned long long k6_rt0 = __builtin_amdgcn_s_memrealtime(); \
                        unsigned long long k6_last = rs_k6_now(); unsigned long long k6p[3] = {0, 0, 0};
#define RS_K6STAMP(i) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = rs_k6_now(); k6_acc[i] += t_ - k6_last; k6_last = t_; \
                           __builtin_amdgcn_sched_barrier(0); } while (0)
#define RS_K6STAMP_TRIPS(active) do { const int m_ = rs_k6p_wave_max((active) ? (int)k6p[1] : 0); k6_acc[9] += m_; k6_acc[10] += m_ > 3 ? m_ - 3 : 0; } while (0)
#define RS_K6STAMP_PHILOX(t0) do { k6_acc[12] += rs_k6p_now() - (t0); } while (0)
#define RS_K6STAMP_EXIT(tmpl, steps) do { if ((threadIdx.x & 63) == 0) { k6_acc[8] = k6p[0]; k6_acc[11] = k6p[2]; k6_acc[14] = __builtin_amdgcn_s_memrealtime() - k6_rt0; k6_acc[15] = (steps); \
                           for (int q = 0; q < RS_K6_NPH; ++q) atomicAdd(&rs_k6_stamp_table[tmpl][q], k6_acc[q]); } } while (0)
#else
#define RS_K6STAMP_DECL
#define RS_K6STAMP(i) do {} while (0)
#define RS_K6STAMP_TRIPS(active) do {} while (0)
#define RS_K6STAMP_PHILOX(t0) do {} while (0)
#define RS_K6STAMP_EXIT(tmpl, steps) do {} while (0)
#endif

template <bool HAS_OBS, int TW>
__device__ __forceinline__ void rs_rollout16_body(const RsParams& P, const RsMlpParams& pa, const RsMlpParams& pc, const rs_rollout_args& R) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* wts = reinterpret_cast<float*>(smem);
    unsigned char* p = smem + sizeof(float) * (size_t)(rs_mlp16_lds_floats(8) + rs_mlp16_lds_floats(1));
    p = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15));
    int* lds_geo = reinterpret_cast<int*>(p);
    uint32_t* lds_adj = reinterpret_cast<uint32_t*>(p + RS_MAX_VERT * RS_WAVE * 4);
    double* lds_d = reinterpret_cast<double*>(p + 2 * RS_MAX_VERT * RS_WAVE * 4);
    float* tile = reinterpret_cast<float*>(p + (HAS_OBS ? (2 * RS_MAX_VERT * RS_WAVE * 4 + RS_MAX_VERT * RS_WAVE * 8) : 0));
    float* lds_rew = tile + RS_WAVE * RS_OBS_DIM;
    uint8_t* lds_done = reinterpret_cast<uint8_t*>(lds_rew + RS_WAVE);
    uint8_t* lds_oob = lds_done + RS_WAVE;
    float* mbox = reinterpret_cast<float*>(lds_oob + RS_WAVE);          // [2 slots][pre 16 x 12 | post 16 x 12 | flags 16]
    f32x4* xch1 = reinterpret_cast<f32x4*>(mbox + 2 * RS_MB_SLOT);      // tile waves: [4 tiles][64 lanes] accumulators of layer 1
    f32x4* xch2 = xch1 + 4 * RS_WAVE;                                   // ... and of layer 2

    RsMlp16<8> ACT; RsMlp16<1> CRT;
    ACT.carve(wts);
    CRT.carve(wts + rs_mlp16_lds_floats(8));
    ACT.fill(pa); CRT.fill(pc);

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, j = lane & 15;
    const bool own = lane < 16;                                   // lane (j, 0) of either wave stands for env slot j
    const int n = blockIdx.x * 16 + j;                            // N % 16 == 0 (checked by the host)
    const int N = P.N, T = R.steps_per_epoch, L = R.steps_per_episode;
    // obstacles: the four lanes (j, 0..3) of an env run its step together (rs_env_step_lane<true, 4>): lane (j, g) takes
    // corner g of every rectangle in the shortest-path loop, every 4th rectangle, two of the eight probe directions
    const int cj = lane >> 4;
    RsGeo g{lds_geo, 0, 0, 0};
    if (HAS_OBS && wave == 0) {
        rs_load_geo(P, n, own, lds_geo, g);
        g.off = __shfl(g.off, j); g.stride = __shfl(g.stride, j); g.n = __shfl(g.n, j);
    }
    __syncthreads();

    using Cfg = RsK6Cfg<HAS_OBS, TW>;
    // tile waves: the wave's first output tile of the actor's hidden layers, and whether it has any
    constexpr int NT = Cfg::tiles_per_wave;
    const int it0 = Cfg::tile_waves == 4 ? (wave == 0 ? 0 : wave == 1 ? 3 : wave - 1) : (wave == 3 ? 2 : 0);
    const bool tiler = Cfg::tile_waves == 4 || (Cfg::tile_waves == 2 && wave >= 2);
    typename RsMlp16<8>::template TileRegs<NT> TR;
    if constexpr (Cfg::tile_waves != 0) {
        if (tiler) ACT.template load_tiles<NT>(TR, it0);
    }

    if (wave != 0) {
        // ---- the critic's wave (1): message t (t = -1: the epoch's first observation) is written by wave 0 before barrier t.
        // Tile waves (1..3): from message t they first compute their tiles of lock-step t + 1's hidden layers, see "Tile waves"
        for (int t = -1; t < T; ++t) {
            __syncthreads();
            const float* M = mbox + (t & 1) * RS_MB_SLOT;
            if constexpr (Cfg::tile_waves != 0) {
                if (t + 1 < T) {                                  // lock-step t + 1 exists: its two exchange barriers
                    f32x4 H1[4], Ht[NT];
                    if (tiler) {
                        // the observation wave 0 goes on with: the post-reset row where the env was cut, as in the row writer below
                        const float* x = M + ((reinterpret_cast<const int*>(M + RS_MB_FLAGS)[j] & 1) ? RS_MB_POST : RS_MB_PRE) + j * RS_IN_PAD + cj;
                        const float b[3] = {x[0], x[4], x[8]};
                        ACT.template tile_layer1<NT>(b, TR, Ht);
#pragma unroll
                        for (int i = 0; i < NT; ++i) xch1[(it0 + i) * RS_WAVE + lane] = Ht[i];
                    }
                    __syncthreads();
                    if (tiler) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) H1[i] = xch1[i * RS_WAVE + lane];
                        ACT.template tile_layer2<NT>(H1, TR, Ht);
#pragma unroll
                        for (int i = 0; i < NT; ++i) xch2[(it0 + i) * RS_WAVE + lane] = Ht[i];
                    }
                    __syncthreads();
                }
                if (wave != 1) continue;
            }
            if constexpr (Cfg::obs_by_wave1) {
                if (t + 1 < T) {                                  // the 16 rows of lock-step t + 1, 704 contiguous bytes
                    float* dst = R.obs + ((size_t)(t + 1) * N + (size_t)blockIdx.x * 16) * RS_OBS_DIM;
                    const int* F = reinterpret_cast<const int*>(M + RS_MB_FLAGS);
                    for (int i = lane; i < 16 * RS_OBS_DIM; i += RS_WAVE) {
                        const int e = i / RS_OBS_DIM, k = i - e * RS_OBS_DIM;
                        dst[i] = M[((F[e] & 1) ? RS_MB_POST : RS_MB_PRE) + e * RS_IN_PAD + k];
                    }
                }
            }
            float xs[RS_IN_PAD];
#pragma unroll
            for (int k = 0; k < RS_IN_PAD; ++k) xs[k] = M[RS_MB_PRE + j * RS_IN_PAD + k];
            float vb;
            { float vv[1]; CRT.forward(xs, vv); vb = vv[0]; }
            const int fl = reinterpret_cast<const int*>(M + RS_MB_FLAGS)[j];          // bit 0: cut, bit 1: boot (both 0 in message -1)
            const bool cut = (fl & 1) != 0, boot = (fl & 2) != 0;
            float v = vb;
            if (__ballot(cut) != 0ull) {                          // the envs that were cut start again from the observation after the reset
#pragma unroll
                for (int k = 0; k < RS_IN_PAD; ++k) xs[k] = M[RS_MB_POST + j * RS_IN_PAD + k];
                float vv[1];
                CRT.forward(xs, vv);
                v = cut ? vv[0] : vb;
            }
            if (own) {
                if (t >= 0) R.last_val[(size_t)t * N + n] = (cut && boot) ? vb : 0.0f;
                if (t + 1 < T) R.val[(size_t)(t + 1) * N + n] = v;
            }
        }
        return;
    }

    float oraw[RS_OBS_DIM];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) oraw[k] = R.cur_obs[(size_t)n * RS_OBS_DIM + k];
    RsWelford W{R.w_count[n], R.w_mean[n], R.w_sq[n], R.w_std[n]};
    int steps = R.steps_in_ep[n];
    float ep_ret = R.ep_ret[n];
    int done_count = 0, oob_count = 0, ep_count = 0;
    double ep_ret_sum = 0.0, ep_len_sum = 0.0, ep_ret_sq = 0.0;
    float ep_ret_max = -INFINITY, ep_ret_min = INFINITY;
    const uint32_t k0 = P.seed, k1 = P.env_id_base + (uint32_t)n;
    // The env's state lives in registers for the whole launch (every lane of wave 0 holds the copy of env slot j; the lanes that
    // step it compute identical results): a global load per lock-step is a full memory latency for the lone wave of a SIMD.  The
    // env arrays are written before a reset, which works on them, re-read after it, and written at the end of the launch.
    // Without Cfg::reg_state the step goes through the arrays (rs_env_step_lane) and E only mirrors what the sampler's Philox
    // counter and the source target need.
    RsEnvRegs E;
    RsAgentRegs S;
    E.load(P, n);
    S.load(P, (size_t)n);                                         // single agent: row 0
    RsMlp16<8>::Regs AR;
    if constexpr (Cfg::tile_waves != 0 && Cfg::reg_weights) {     // of the full set, the output layer's operands only
        ACT.load_w3(AR.w3);
#pragma unroll
        for (int i = 0; i < 32; ++i) AR.w3[i >> 4][i & 15] = RsMlp16<8>::park(AR.w3[i >> 4][i & 15]);
    } else if constexpr (Cfg::reg_weights) ACT.load(AR);

    float xo[RS_IN_PAD], xs[RS_IN_PAD];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) xo[k] = oraw[k];
    xo[0] = W.standardize(oraw[0]);
    xo[11] = 1.0f;                                                // constant input carrying the layer-1 bias
    rs_bcast_x16(xo, xs);
    {   // message -1: the epoch's first observation (no flags)
        float* M = mbox + RS_MB_SLOT;
        if (own) {
#pragma unroll
            for (int k = 0; k < RS_IN_PAD; ++k) M[RS_MB_PRE + j * RS_IN_PAD + k] = xo[k];
            reinterpret_cast<int*>(M + RS_MB_FLAGS)[j] = 0;
        }
    }
    __syncthreads();

    RsOut O;
    O.obs_row = tile + j * RS_OBS_DIM;
    O.reward = lds_rew + j - (size_t)n;
    O.team = nullptr;
    O.done = lds_done + j - (size_t)n;
    O.oob = lds_oob + j - (size_t)n;
    O.oobc = nullptr; O.blocked = nullptr; O.collision = nullptr;

    RS_K6STAMP_DECL
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)t * N + n;
        float* M = mbox + (t & 1) * RS_MB_SLOT;
        float lg[8];
        u32x4 ph{0u, 0u, 0u, 0u};
        if constexpr (Cfg::group_draw) {                          // the counters are known before the logits are
#ifdef RS_K6_STAMPS
            const unsigned long long p0 = rs_k6p_now();
#endif
            ph = philox4x32_10(cj ? (uint32_t)(cj - 1) : 0u, E.tstep, E.episode, cj ? RS_STREAM_STEP : RS_STREAM_ACT, k0, k1);
            RS_K6STAMP_PHILOX(p0);
            RS_K6STAMP(13);                                      // (kept out of "hidden layers")
        }
        {
            f32x4 H2[4];
            if constexpr (Cfg::tile_waves != 0) {
                if constexpr (Cfg::tile_waves == 4) {
                    f32x4 Ht[NT];
                    const float b[3] = {(cj == 0) ? xs[0] : (cj == 1) ? xs[1] : (cj == 2) ? xs[2] : xs[3],
                                        (cj == 0) ? xs[4] : (cj == 1) ? xs[5] : (cj == 2) ? xs[6] : xs[7],
                                        (cj == 0) ? xs[8] : (cj == 1) ? xs[9] : (cj == 2) ? xs[10] : xs[11]};
                    ACT.template tile_layer1<NT>(b, TR, Ht);
                    xch1[it0 * RS_WAVE + lane] = Ht[0];
                    RS_K6STAMP(0);
                    __syncthreads();
                    f32x4 H1[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) H1[i] = xch1[i * RS_WAVE + lane];
                    RS_K6STAMP(16);                              // (inside hidden layers: the H1 exchange)
                    ACT.template tile_layer2<NT>(H1, TR, Ht);
                    xch2[it0 * RS_WAVE + lane] = Ht[0];
                    RS_K6STAMP(0);
                    __syncthreads();
                } else {                                         // waves 2 and 3 compute; the two exchange barriers of the lock-step
                    RS_K6STAMP(0);
                    __syncthreads();
                    RS_K6STAMP(16);
                    __syncthreads();
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) H2[i] = xch2[i * RS_WAVE + lane];
                RS_K6STAMP(17);                                  // (inside hidden layers: the H2 exchange)
            } else {
                ACT.template hidden<Cfg::reg_weights>(xs, H2, AR);
                RS_K6STAMP(0);                                   // hidden layers
            }
            if constexpr (!Cfg::mfma_out) ACT.output(H2, lg);
            else if constexpr (Cfg::reg_weights) ACT.output_mfma(H2, lg, AR.w3);
            else { float w3[2][16]; ACT.load_w3(w3); ACT.output_mfma(H2, lg, w3); }
            RS_K6STAMP(1);                                       // output layer
        }
        int a = 0;
        float logp = 0.0f;
        if (own) {
            float mx = lg[0];
#pragma unroll
            for (int q = 1; q < 8; ++q) mx = fmaxf(mx, lg[q]);
            float se = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) se += __expf(lg[q] - mx);
            const float lse = __logf(se);
            if constexpr (!Cfg::group_draw) {
#ifdef RS_K6_STAMPS
                const unsigned long long p0 = rs_k6p_now();
#endif
                ph = philox4x32_10(0u, E.tstep, E.episode, RS_STREAM_ACT, k0, k1);
                RS_K6STAMP_PHILOX(p0);
            }
            const float u = (float)(ph.x >> 8) * (1.0f / 16777216.0f);
            float cdf = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float lpq = (lg[q] - mx) - lse;
                cdf += __expf(lpq);
                if (q < 7) a += (cdf <= u) ? 1 : 0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) logp = (a == q) ? ((lg[q] - mx) - lse) : logp;
            if constexpr (!Cfg::obs_by_wave1) {
#pragma unroll
                for (int k = 0; k < RS_OBS_DIM; ++k) tile[lane * RS_OBS_DIM + k] = xo[k];
            }
        }
        __builtin_amdgcn_wave_barrier();                         // (one wave: its LDS operations are ordered; this only pins the compiler)
        RS_K6STAMP(2);                                           // softmax + draw
        if constexpr (!Cfg::obs_by_wave1) {
            float* dst = R.obs + ((size_t)t * N + (size_t)blockIdx.x * 16) * RS_OBS_DIM;
            for (int i = lane; i < 16 * RS_OBS_DIM; i += RS_WAVE) dst[i] = tile[i];
        }
        __builtin_amdgcn_wave_barrier();
        bool cut = false;
        bool over = false, boot = false, ended = t == T - 1;
        if (own) {
            R.act[row] = (int64_t)a;
            R.logp[row] = logp;
            R.source_tar[row * 2 + 0] = (float)E.sx;
            R.source_tar[row * 2 + 1] = (float)E.sy;
        }
        RS_K6STAMP(3);                                           // buffer stores
        // group_draw: all four lanes of an env step it, with identical values (the LDS outputs are duplicate addresses, as with
        // obstacles), so that lanes 1..3 hold the rate and their candidates of the measurement draw
        constexpr bool STEP_ALL = HAS_OBS || Cfg::group_draw;
        if (STEP_ALL || own) {
            const int a_env = STEP_ALL ? __shfl(a, j) : a;
            if constexpr (Cfg::reg_state) {
                double max_reward = 0.0;
                bool have_max = false;
#ifdef RS_STEP_STAMPS
                RS_ESTAMP_DECL
#endif
                rs_agent_step_core<HAS_OBS, HAS_OBS ? 4 : 1>(P, g, n, 0, a_env, false, E, S, O, max_reward, have_max, cj RS_ESTAMP_ARG,
                                                             Cfg::group_draw ? &ph : nullptr);
            } else {
                rs_env_step_lane<HAS_OBS, HAS_OBS ? 4 : 1>(P, g, n, [&](int) -> int { return a_env; }, O, false, cj);
            }
            E.iter_count += 1;
            E.tstep += 1;                                        // the env advanced its step counter
        }
        RS_K6STAMP_TRIPS(STEP_ALL || own);
        RS_K6STAMP(4);                                           // env step
        if (own) {
            const float r = lds_rew[lane];
            const bool terminal = lds_done[lane] != 0;
            oob_count += lds_oob[lane];
            R.rew[row] = r;
            ep_ret += r;
            steps += 1;
            done_count += terminal ? 1 : 0;
            const bool timeout = steps == L;
            over = terminal || timeout;
            cut = over || ended;
            boot = timeout || ended;
#pragma unroll
            for (int k = 0; k < RS_OBS_DIM; ++k) oraw[k] = tile[lane * RS_OBS_DIM + k];
            W.update((double)oraw[0]);
#pragma unroll
            for (int k = 1; k < RS_OBS_DIM; ++k) xo[k] = oraw[k];
            xo[0] = W.standardize(oraw[0]);
            // the critic's message: the observation the bootstrap value is taken on, and whether it is
#pragma unroll
            for (int k = 0; k < RS_IN_PAD; ++k) M[RS_MB_PRE + j * RS_IN_PAD + k] = xo[k];
            reinterpret_cast<int*>(M + RS_MB_FLAGS)[j] = (cut ? 1 : 0) | (boot ? 2 : 0);
            R.cut[row] = cut ? 1 : 0;
            if (over) {
                ep_ret_sum += (double)ep_ret; ep_len_sum += (double)steps; ep_count += 1;
                ep_ret_sq += (double)ep_ret * (double)ep_ret;
                ep_ret_max = fmaxf(ep_ret_max, ep_ret); ep_ret_min = fminf(ep_ret_min, ep_ret);
            }
        }
        RS_K6STAMP(5);                                           // Welford + mailbox message
        if (HAS_OBS ? (__shfl((int)cut, j) != 0) : cut) {        // obstacles: the env's four lanes reset it together
            if (ended) P.epoch_end[n] = 1;
            if constexpr (Cfg::reg_state) { S.store(P, (size_t)n); E.store(P, n); }
            if constexpr (HAS_OBS) rs_env_reset_lane<true, 4>(P, g, n, lds_geo, lds_adj, lds_d, tile + j * RS_OBS_DIM, O, j, cj);
            else rs_env_reset_lane<false>(P, g, n, lds_geo, lds_adj, lds_d, tile + lane * RS_OBS_DIM, O);
            E.load(P, n);                                        // new episode: new source, new Philox counters
            if constexpr (Cfg::reg_state) S.load(P, (size_t)n);
        }
        if constexpr (Cfg::group_draw && !HAS_OBS) {             // the reset ran in lane (j, 0) alone: its new state to the env's other lanes
            if (__ballot(cut) != 0ull) { E.from_lane(j); S.from_lane(j); }
        }
        if (own) {
            if (cut) {
                W.reset();
#pragma unroll
                for (int k = 0; k < RS_OBS_DIM; ++k) oraw[k] = tile[lane * RS_OBS_DIM + k];
                W.update((double)oraw[0]);
#pragma unroll
                for (int k = 1; k < RS_OBS_DIM; ++k) xo[k] = oraw[k];
                xo[0] = W.standardize(oraw[0]);
                steps = 0;
                ep_ret = 0.0f;
#pragma unroll
                for (int k = 0; k < RS_IN_PAD; ++k) M[RS_MB_POST + j * RS_IN_PAD + k] = xo[k];
            }
        }
        RS_K6STAMP(6);                                           // reset
        rs_bcast_x16(xo, xs);
        __syncthreads();                                          // message t is complete; wave 1 takes it from here
        RS_K6STAMP(7);                                           // broadcast + barrier
    }
    RS_K6STAMP_EXIT(HAS_OBS ? 1 : 0, (unsigned long long)T);
    if constexpr (Cfg::reg_state) {
        if (HAS_OBS || own) { S.store(P, (size_t)n); E.store(P, n); }
    }
    if (own) {
#pragma unroll
        for (int k = 0; k < RS_OBS_DIM; ++k) R.cur_obs[(size_t)n * RS_OBS_DIM + k] = oraw[k];
        R.w_count[n] = W.count; R.w_mean[n] = W.mean; R.w_sq[n] = W.sq; R.w_std[n] = W.std;
        R.steps_in_ep[n] = steps;
        R.ep_ret[n] = ep_ret;
        R.done_count[n] = done_count; R.oob_count[n] = oob_count; R.ep_count[n] = ep_count;
        R.ep_ret_sum[n] = ep_ret_sum; R.ep_len_sum[n] = ep_len_sum;
        R.ep_ret_sq_sum[n] = ep_ret_sq; R.ep_ret_max[n] = ep_ret_max; R.ep_ret_min[n] = ep_ret_min;
    }
}

template <bool HAS_OBS>
__global__ void __launch_bounds__(RsK6Cfg<HAS_OBS>::waves * RS_WAVE) rs_rollout16_kernel(RsParams P, RsMlpParams pa, RsMlpParams pc, rs_rollout_args R) {
    rs_rollout16_body<HAS_OBS, RsK6Cfg<HAS_OBS>::tile_waves>(P, pa, pc, R);
}
// Without obstacles and with more workgroups than CUs (more than 4096 envs on 256 CUs): the two-wave workgroup, of which a CU holds two
// at once.  Four-wave workgroups have a CU each and would run in twice as many rounds, which costs more than the tile waves save.
__global__ void __launch_bounds__(2 * RS_WAVE) rs_rollout16_wide_kernel(RsParams P, RsMlpParams pa, RsMlpParams pc, rs_rollout_args R) {
    rs_rollout16_body<false, 0>(P, pa, pc, R);
}

// rs_cnn_eval.hip -- the policy heads of a RAD-TEAM (CNN) team in the Monte-Carlo evaluation's lock-step
// (radiation_ppo_amd/evaluate.py: run_test_environments_cnn_team), one launch for every agent: grid = (64-image tiles, agent).
//
// rs_cnn_team_eval_head: a2 [A][N][2704] (the team trunk's output, rs_cnn.hip) -> Linear(2704, 32) -> ReLU -> Linear(32, 16) -> ReLU ->
// Linear(16, 8) -> log-softmax -> inverse-CDF draw -> rs_step's action rows, 8 (idle) on the lanes whose episode has ended.
//
// The first layer is 173 kFLOP on 10.8 KB per image and agent, the only part with weight: y1 = a2 W1^T runs on v_mfma_f32_32x32x2_f32
// (exact f32, an fmaf chain over k).  A = W1 (row = output neuron), B = a2 (column = image); both matrices are row-major over k and
// both operands have the lane pattern (row l & 31, k-half l >> 5), so one loading scheme serves both: a lane reads float4s along ITS
// row.  A workgroup is four waves on the same 64 images (two 32-image B tiles share every A fragment: W1 comes from L2 once per 64
// images); wave w owns k in [676 w, 676 w + 676) = 21 pieces of 32 floats, of which its lane halves take 16 each (64 contiguous bytes
// per lane and operand: the two halves of a row read one 128-byte piece), and a last float4 that the lower half takes while the upper
// feeds zeros (2704 = 8 x 338, and 338 is no multiple of 4).  The four partial sums meet in LDS and are added in wave order, then the bias: no atomics, the
// bits of an image's result depend on neither N nor the grid.  Wave 0 then runs rs_cnn_head_kernel<8>'s arithmetic (rs_cnn_loss.hip),
// operation for operation, one image per lane, its weights through the scalar unit.
//
// Not fused into the trunk on purpose: a trunk workgroup holds 3 images, so W1 (346 KB per agent) would be re-read from L2 once per 3
// images = 115 KB per image, where the a2 round trip it would save is 21.6 KB per image.
//
// rs_cnn_sized_team_eval_head (run_test_environments_cnn_team_sized): the same scheme at a run-time depth 16 p p for the tiled trunk's
// maps of any side; it shares the MFMA step and everything behind the k loop (eh_step, eh_finish) and has a kernel of its own.
//
// rs_cnn_team_step_head (CNNCollector._step_glued, radiation_ppo_amd/ppo_cnn.py): the same first layer for every actor AND every critic
// of a team in training, one launch per policy round; behind the evaluation kernels.
//
// rs_cnn_sized_team_step_head: that round at a run-time depth (walls-off maps), the first layer split over k across workgroups with a
// fixed-order second stage; at the end of this file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_cnn_head.hpp"

namespace {

constexpr int FLAT = 2704, H1 = RS_HEAD_H1, H2 = RS_HEAD_H2, NACT = RS_HEAD_NA;      // (csrc/rs_cnn_head.hpp)
constexpr int EH_WAVES = 4, EH_NT = 64 * EH_WAVES;
constexpr int EH_TILE = 64;                         // images per workgroup: two MFMA column tiles
constexpr int EH_KW = FLAT / EH_WAVES;              // 676 k per wave
constexpr int EH_PIECES = EH_KW / 32;               // 21 pieces of 32 floats per wave (16 per lane half), then 4 floats
constexpr int EH_ROW = H1 + 4;                      // LDS row of an image's 32 partial sums, padded (16-byte aligned rows, banks spread)
static_assert(FLAT % (4 * EH_WAVES) == 0 && EH_KW == 32 * EH_PIECES + 4 && EH_PIECES % 2 == 1, "21 pieces and one float4 per wave");

typedef float v16f __attribute__((ext_vector_type(16)));
typedef const float __attribute__((address_space(4))) * eh_cmem_t;
__device__ __forceinline__ eh_cmem_t eh_cmem(const float* p) { return (eh_cmem_t)(uintptr_t)p; }

// every agent's head pointers travel in the kernel's argument block (8 agents x 6 pointers = 384 bytes)
struct EhNets {
    rs_cnn_head_params head[RS_MAX_AGENTS];
};

// eight MFMAs: one float4 of W1 (A operand) against the same float4 of the two 32-image tiles (B operands)
__device__ __forceinline__ void eh_step(v16f& acc0, v16f& acc1, const float4& w, const float4& a, const float4& b) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, a.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, b.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, a.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, b.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, a.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, b.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, a.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, b.w, acc1, 0, 0, 0);
}

// eh_finish, and ts_hidden / ts_draw further down, write out the arithmetic of csrc/rs_cnn_head.hpp, which rs_cnn_head_kernel and
// sk_heads_kernel run; keep them in step by hand.  Rebuilt from the shared pieces (with the evaluation kernel calling ts_k2704) the
// evaluation heads kept their 164 / 196 registers and their bits, but the fused evaluation at 1000 lanes timed 0.1277 ms against
// 0.1275 ms + 0.0001 ms of spread with one agent and 0.3134 ms against 0.3125 ms + 0.0008 ms with four (three alternated rounds), and
// rs_cnn_team_step_head_kernel's bootstrap round with eight critics 0.0824 ms against 0.0810 ms + 0.0009 ms (five rounds): outside the
// rule (profiles/policy_pieces_timing.txt).
// Behind the k loop, the same for every depth: the waves' partial sums meet in LDS; wave 0 adds them in wave order, then the bias, and
// runs rs_cnn_head_kernel<8>'s arithmetic, the draw and the idle rule, one image per lane.
__device__ __forceinline__ void eh_finish(float (*part)[EH_TILE][EH_ROW], const v16f& acc0, const v16f& acc1, const rs_cnn_head_params& P,
                                          int ag, int A, int n0, const float* __restrict__ u, const uint8_t* __restrict__ alive,
                                          int8_t* __restrict__ act8, int64_t* __restrict__ act, float* __restrict__ logp,
                                          float* __restrict__ y1_out, int N) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    // C layout: register i of lane (r, h) is neuron (i & 3) + 8 (i >> 2) + 4 h of image r
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(&part[wave][r][8 * g + 4 * h]) = make_float4(acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]);
        *reinterpret_cast<float4*>(&part[wave][32 + r][8 * g + 4 * h]) = make_float4(acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]);
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- one image per lane: the four k-quarters in wave order, then the bias; behind it rs_cnn_head_kernel<8>
    const int n = n0 + lane;
    const bool live = n < N;
    const int nc = live ? n : N - 1;
    const eh_cmem_t b1 = eh_cmem(P.b1), w2 = eh_cmem(P.w2), b2 = eh_cmem(P.b2), w3 = eh_cmem(P.w3), b3 = eh_cmem(P.b3);
    float h1[H1];
#pragma unroll
    for (int k = 0; k < H1; k += 4) {
        float4 s = *reinterpret_cast<const float4*>(&part[0][lane][k]);
#pragma unroll
        for (int w = 1; w < EH_WAVES; ++w) {
            const float4 q = *reinterpret_cast<const float4*>(&part[w][lane][k]);
            s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
        }
        s.x += b1[k]; s.y += b1[k + 1]; s.z += b1[k + 2]; s.w += b1[k + 3];
        if (y1_out && live) *reinterpret_cast<float4*>(y1_out + ((size_t)ag * N + n) * H1 + k) = s;
        h1[k] = fmaxf(s.x, 0.0f); h1[k + 1] = fmaxf(s.y, 0.0f); h1[k + 2] = fmaxf(s.z, 0.0f); h1[k + 3] = fmaxf(s.w, 0.0f);
    }
    float h2[H2];
#pragma unroll
    for (int o = 0; o < H2; ++o) {
        float s = b2[o];
#pragma unroll
        for (int k = 0; k < H1; ++k) s = __builtin_fmaf(w2[o * H1 + k], h1[k], s);
        h2[o] = fmaxf(s, 0.0f);
    }
    float lg[NACT];
#pragma unroll
    for (int o = 0; o < NACT; ++o) {
        float s = b3[o];
#pragma unroll
        for (int k = 0; k < H2; ++k) s = __builtin_fmaf(w3[o * H2 + k], h2[k], s);
        lg[o] = s;
    }
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NACT; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NACT; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
    const float uu = u[(size_t)nc * A + ag];
    float cdf = 0.0f, lp_sel = (lg[0] - mx) - lse;
    int a = 0;
#pragma unroll
    for (int o = 0; o < NACT; ++o) {
        const float lp = (lg[o] - mx) - lse;
        cdf += expf(lp);
        if (o < NACT - 1 && cdf <= uu) a = o + 1;
    }
#pragma unroll
    for (int o = 1; o < NACT; ++o) if (a == o) lp_sel = (lg[o] - mx) - lse;
    if (live) {
        if (act) act[(size_t)ag * N + n] = a;
        if (logp) logp[(size_t)ag * N + n] = lp_sel;
        act8[(size_t)n * A + ag] = alive[n] != 0 ? (int8_t)a : (int8_t)8;     // finished episodes idle in place
    }
}

__global__ void __launch_bounds__(EH_NT) rs_cnn_team_eval_head_kernel(EhNets nets, int A, const float* __restrict__ a2,
                                                                      const float* __restrict__ u, const uint8_t* __restrict__ alive,
                                                                      int8_t* __restrict__ act8, int64_t* __restrict__ act,
                                                                      float* __restrict__ logp, float* __restrict__ y1_out, int N) {
    __shared__ __align__(16) float part[EH_WAVES][EH_TILE][EH_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int ag = blockIdx.y;
    const rs_cnn_head_params P = nets.head[ag];
    const int n0 = blockIdx.x * EH_TILE;
    // rows past the last image read the last image's (their sums are dropped)
    const int na = n0 + r < N ? n0 + r : N - 1, nb = n0 + 32 + r < N ? n0 + 32 + r : N - 1;
    const float* wp = P.w1 + (size_t)r * FLAT + wave * EH_KW + 16 * h;
    const float* xa = a2 + ((size_t)ag * N + na) * FLAT + wave * EH_KW + 16 * h;
    const float* xb = a2 + ((size_t)ag * N + nb) * FLAT + wave * EH_KW + 16 * h;
    v16f acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
    auto step = [&](const float4& w, const float4& a, const float4& b) { eh_step(acc0, acc1, w, a, b); };
    // a piece = 32 floats of the wave's k range: 16 per lane half, four float4s per operand and lane (64 contiguous bytes of its row).
    // Two pieces live in registers: piece g + 2 is requested as soon as piece g has been issued to the matrix cores, so ~12 KB per
    // wave are in flight under the 32 MFMAs (2048 cycles) of a piece -- one request per trip left the kernel waiting on HBM latency
    struct Piece { float4 w[4], a[4], b[4]; };
    auto fetch = [&](Piece& q, int g) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q.w[i] = *reinterpret_cast<const float4*>(wp + 32 * g + 4 * i);
            q.a[i] = *reinterpret_cast<const float4*>(xa + 32 * g + 4 * i);
            q.b[i] = *reinterpret_cast<const float4*>(xb + 32 * g + 4 * i);
        }
    };
    auto consume = [&](const Piece& q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) step(q.w[i], q.a[i], q.b[i]);
    };
    Piece p0, p1;
    fetch(p0, 0);
    fetch(p1, 1);
#pragma unroll 1
    for (int g = 0; g < EH_PIECES - 1; g += 2) {                    // pieces 0 .. 19 in pairs, piece 20 behind the loop
        consume(p0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(p0, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        consume(p1);
        __builtin_amdgcn_sched_barrier(0);
        fetch(p1, g + 3 < EH_PIECES ? g + 3 : EH_PIECES - 1);       // (the last trip re-requests piece 20; it is dropped)
        __builtin_amdgcn_sched_barrier(0);
    }
    consume(p0);
    {   // the range's last four floats, 672 .. 675: on the lower half; the upper half re-reads floats of piece 20 and feeds zeros
        const int o = 32 * EH_PIECES - 32 * h;
        float4 w = *reinterpret_cast<const float4*>(wp + o);
        float4 a = *reinterpret_cast<const float4*>(xa + o);
        float4 b = *reinterpret_cast<const float4*>(xb + o);
        if (h) { w = make_float4(0.f, 0.f, 0.f, 0.f); a = w; b = w; }
        step(w, a, b);
    }
    eh_finish(part, acc0, acc1, P, ag, A, n0, u, alive, act8, act, logp, y1_out, N);
}

// ------------------------------------------------------------------------------------------------
// rs_cnn_sized_team_eval_head: the same scheme with the depth as an argument, flat = 16 p p (p = 4..128: the tiled trunk's output,
// rs_cnn_sized.hip; 85 264 at 147 x 147 maps).  Wave w owns k in [kw w, kw w + kw), kw = flat / 4 = 4 p p: np = kw / 32 whole pieces
// (at least 2: p = 4 gives 2, p = 5 gives 3, p = 73 gives 666), which the two-pieces-in-flight loop takes in pairs with the odd one
// behind it, and a tail of kw % 32 floats: 0 (p % 4 == 0), 16 (p % 4 == 2: two float4 steps, floats 0..7 on the lower lane half and 8..15
// on the upper) or 4 (p odd: one float4 step on the lower half while the upper feeds zeros, as the 2704 kernel's).  Every row of a2 and
// W1 is 64-byte aligned and every wave's range 16-byte aligned, so all loads are float4s.  A kernel of its own: the 2704 kernel keeps
// its compile-time trip counts and its measured numbers.  No scratch; 196 VGPRs with the accumulators (two waves per SIMD, <= 256);
// 4 x 64 x 36 floats of LDS.
__global__ void __launch_bounds__(EH_NT) rs_cnn_sized_team_eval_head_kernel(EhNets nets, int A, int flat, const float* __restrict__ a2,
                                                                            const float* __restrict__ u, const uint8_t* __restrict__ alive,
                                                                            int8_t* __restrict__ act8, int64_t* __restrict__ act,
                                                                            float* __restrict__ logp, float* __restrict__ y1_out, int N) {
    __shared__ __align__(16) float part[EH_WAVES][EH_TILE][EH_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int ag = blockIdx.y;
    const rs_cnn_head_params P = nets.head[ag];
    const int n0 = blockIdx.x * EH_TILE;
    const int kw = flat / EH_WAVES, np = kw / 32, tail = kw - 32 * np;
    // rows past the last image read the last image's (their sums are dropped)
    const int na = n0 + r < N ? n0 + r : N - 1, nb = n0 + 32 + r < N ? n0 + 32 + r : N - 1;
    const float* wp = P.w1 + (size_t)r * flat + (size_t)wave * kw;
    const float* xa = a2 + ((size_t)ag * N + na) * flat + (size_t)wave * kw;
    const float* xb = a2 + ((size_t)ag * N + nb) * flat + (size_t)wave * kw;
    v16f acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
    struct Piece { float4 w[4], a[4], b[4]; };
    auto fetch = [&](Piece& q, int g) {                               // the lane half's 16 floats of piece g
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = 32 * g + 16 * h + 4 * i;
            q.w[i] = *reinterpret_cast<const float4*>(wp + o);
            q.a[i] = *reinterpret_cast<const float4*>(xa + o);
            q.b[i] = *reinterpret_cast<const float4*>(xb + o);
        }
    };
    auto consume = [&](const Piece& q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) eh_step(acc0, acc1, q.w[i], q.a[i], q.b[i]);
    };
    Piece p0, p1;
    fetch(p0, 0);
    fetch(p1, 1);
    int g = 0;
#pragma unroll 1
    for (; g + 2 < np; g += 2) {                                      // p0 holds piece g, p1 piece g + 1, both with a successor
        consume(p0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(p0, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        consume(p1);
        __builtin_amdgcn_sched_barrier(0);
        fetch(p1, g + 3 < np ? g + 3 : np - 1);                       // (an odd np re-requests its last piece; it is dropped)
        __builtin_amdgcn_sched_barrier(0);
    }
    consume(p0);                                                      // the last two pieces, or the last one
    if (g + 1 < np) consume(p1);
    if (tail == 16) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = 32 * np + 8 * h + 4 * i;
            eh_step(acc0, acc1, *reinterpret_cast<const float4*>(wp + o), *reinterpret_cast<const float4*>(xa + o),
                    *reinterpret_cast<const float4*>(xb + o));
        }
    } else if (tail == 4) {                                           // both halves read the float4; the upper half feeds zeros
        const int o = 32 * np;
        float4 w = *reinterpret_cast<const float4*>(wp + o);
        float4 a = *reinterpret_cast<const float4*>(xa + o);
        float4 b = *reinterpret_cast<const float4*>(xb + o);
        if (h) { w = make_float4(0.f, 0.f, 0.f, 0.f); a = w; b = w; }
        eh_step(acc0, acc1, w, a, b);
    }
    eh_finish(part, acc0, acc1, P, ag, A, n0, u, alive, act8, act, logp, y1_out, N);
}

// ------------------------------------------------------------------------------------------------
// rs_cnn_team_step_head: the heads of a team's TRAINING round (CNNCollector._step_glued), one launch for every actor and every critic:
// grid = (64-image tiles, row), rows 0 .. A - 1 the actors, rows A .. A + C - 1 the critics (C = 1: a global critic, its value goes to every
// agent's row; C = A: critic c serves agent c).  Every row runs the evaluation kernel's first layer -- the same k ranges, pieces and MFMA
// order, the four k-quarters added in wave order, then the bias: an actor row's y1, action and log-probability are
// rs_cnn_team_eval_head's bits -- and behind it rs_cnn_head_kernel's arithmetic: <8> with the draw on the actor rows (no idle rule: act8 is
// the drawn action), <1> on the critic rows.  Results go to the collector's row buffer f [A][3][N] = {logp, value, bootstrap value}
// (what rs_store_rows reads).  The bootstrap round launches the critic rows alone (row0 = A) under a mask that is empty on most
// lock-steps: a workgroup whose 64 envs are all masked out returns before it has requested a byte of W1 or a2.
// The k loop and the pieces behind it are copies of the evaluation kernel's (the lambdas above, eh_finish) and not shared with it:
// called from a common inline function the evaluation kernel keeps its registers but comes out in another instruction order, and its
// measured numbers are the ones DESIGN.md quotes.  eh_step and the constants are shared.
struct TsNets {
    rs_cnn_head_params net[2 * RS_MAX_AGENTS];      // [0, A): the actors; [A, A + C): the critics (768 bytes of the argument block)
};

__device__ __forceinline__ void ts_meet(float (*part)[EH_TILE][EH_ROW], const v16f& acc0, const v16f& acc1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    // C layout: register i of lane (r, h) is neuron (i & 3) + 8 (i >> 2) + 4 h of image r
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(&part[wave][r][8 * g + 4 * h]) = make_float4(acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]);
        *reinterpret_cast<float4*>(&part[wave][32 + r][8 * g + 4 * h]) = make_float4(acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]);
    }
    __syncthreads();
}

// y1 of the lane's image: the four k-quarters in wave order, then the bias (y1_row: where to keep it, or NULL); ReLU -> Linear(32, 16) -> ReLU
__device__ __forceinline__ void ts_hidden(float (*part)[EH_TILE][EH_ROW], const rs_cnn_head_params& P, int lane, float* __restrict__ y1_row,
                                          float (&h2)[H2]) {
    const eh_cmem_t b1 = eh_cmem(P.b1), w2 = eh_cmem(P.w2), b2 = eh_cmem(P.b2);
    float h1[H1];
#pragma unroll
    for (int k = 0; k < H1; k += 4) {
        float4 s = *reinterpret_cast<const float4*>(&part[0][lane][k]);
#pragma unroll
        for (int w = 1; w < EH_WAVES; ++w) {
            const float4 q = *reinterpret_cast<const float4*>(&part[w][lane][k]);
            s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
        }
        s.x += b1[k]; s.y += b1[k + 1]; s.z += b1[k + 2]; s.w += b1[k + 3];
        if (y1_row) *reinterpret_cast<float4*>(y1_row + k) = s;
        h1[k] = fmaxf(s.x, 0.0f); h1[k + 1] = fmaxf(s.y, 0.0f); h1[k + 2] = fmaxf(s.z, 0.0f); h1[k + 3] = fmaxf(s.w, 0.0f);
    }
#pragma unroll
    for (int o = 0; o < H2; ++o) {
        float s = b2[o];
#pragma unroll
        for (int k = 0; k < H1; ++k) s = __builtin_fmaf(w2[o * H1 + k], h1[k], s);
        h2[o] = fmaxf(s, 0.0f);
    }
}

// Linear(16, 8) -> log-softmax -> the inverse-CDF draw on uu: the action and its log-probability
__device__ __forceinline__ void ts_draw(const rs_cnn_head_params& P, const float (&h2)[H2], float uu, int& a, float& lp_sel) {
    const eh_cmem_t w3 = eh_cmem(P.w3), b3 = eh_cmem(P.b3);
    float lg[NACT];
#pragma unroll
    for (int o = 0; o < NACT; ++o) {
        float s = b3[o];
#pragma unroll
        for (int k = 0; k < H2; ++k) s = __builtin_fmaf(w3[o * H2 + k], h2[k], s);
        lg[o] = s;
    }
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NACT; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NACT; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
    float cdf = 0.0f;
    lp_sel = (lg[0] - mx) - lse;
    a = 0;
#pragma unroll
    for (int o = 0; o < NACT; ++o) {
        const float lp = (lg[o] - mx) - lse;
        cdf += expf(lp);
        if (o < NACT - 1 && cdf <= uu) a = o + 1;
    }
#pragma unroll
    for (int o = 1; o < NACT; ++o) if (a == o) lp_sel = (lg[o] - mx) - lse;
}

// one wave's quarter of the 2704-deep first layer: rs_cnn_team_eval_head_kernel's loop (see there), two pieces in flight
__device__ __forceinline__ void ts_k2704(const float* wp, const float* xa, const float* xb, int h, v16f& acc0, v16f& acc1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
    struct Piece { float4 w[4], a[4], b[4]; };
    auto fetch = [&](Piece& q, int g) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q.w[i] = *reinterpret_cast<const float4*>(wp + 32 * g + 4 * i);
            q.a[i] = *reinterpret_cast<const float4*>(xa + 32 * g + 4 * i);
            q.b[i] = *reinterpret_cast<const float4*>(xb + 32 * g + 4 * i);
        }
    };
    auto consume = [&](const Piece& q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) eh_step(acc0, acc1, q.w[i], q.a[i], q.b[i]);
    };
    Piece p0, p1;
    fetch(p0, 0);
    fetch(p1, 1);
#pragma unroll 1
    for (int g = 0; g < EH_PIECES - 1; g += 2) {                    // pieces 0 .. 19 in pairs, piece 20 behind the loop
        consume(p0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(p0, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        consume(p1);
        __builtin_amdgcn_sched_barrier(0);
        fetch(p1, g + 3 < EH_PIECES ? g + 3 : EH_PIECES - 1);       // (the last trip re-requests piece 20; it is dropped)
        __builtin_amdgcn_sched_barrier(0);
    }
    consume(p0);
    {   // the range's last four floats, 672 .. 675: on the lower half; the upper half re-reads floats of piece 20 and feeds zeros
        const int o = 32 * EH_PIECES - 32 * h;
        float4 w = *reinterpret_cast<const float4*>(wp + o);
        float4 a = *reinterpret_cast<const float4*>(xa + o);
        float4 b = *reinterpret_cast<const float4*>(xb + o);
        if (h) { w = make_float4(0.f, 0.f, 0.f, 0.f); a = w; b = w; }
        eh_step(acc0, acc1, w, a, b);
    }
}

__global__ void __launch_bounds__(EH_NT) rs_cnn_team_step_head_kernel(TsNets nets, int A, int C, int row0, int slot,
                                                                      const float* __restrict__ a2_actor, const float* __restrict__ a2_critic,
                                                                      const float* __restrict__ u, int64_t* __restrict__ act,
                                                                      float* __restrict__ f, int8_t* __restrict__ act8,
                                                                      const uint8_t* __restrict__ mask, float* __restrict__ y1_out, int N) {
    __shared__ __align__(16) float part[EH_WAVES][EH_TILE][EH_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int y = row0 + blockIdx.y;
    const int n0 = blockIdx.x * EH_TILE;
    const int n = n0 + lane;
    // every wave looks at the same 64 flags, so the four of them agree: nothing to do for this tile -> all leave before the barrier
    const bool on = n < N && (mask == nullptr || mask[n] != 0);
    if (!__any(on)) return;
    const bool actor = y < A;
    const rs_cnn_head_params P = nets.net[y];
    const float* a2 = actor ? a2_actor + (size_t)y * N * FLAT : a2_critic + (size_t)(y - A) * N * FLAT;
    // rows past the last image read the last image's (their sums are dropped)
    const int na = n0 + r < N ? n0 + r : N - 1, nb = n0 + 32 + r < N ? n0 + 32 + r : N - 1;
    const float* wp = P.w1 + (size_t)r * FLAT + wave * EH_KW + 16 * h;
    const float* xa = a2 + (size_t)na * FLAT + wave * EH_KW + 16 * h;
    const float* xb = a2 + (size_t)nb * FLAT + wave * EH_KW + 16 * h;
    v16f acc0, acc1;
    ts_k2704(wp, xa, xb, h, acc0, acc1);
    ts_meet(part, acc0, acc1);
    if (wave != 0) return;
    const int nc = n < N ? n : N - 1;
    float h2[H2];
    ts_hidden(part, P, lane, y1_out && on ? y1_out + ((size_t)y * N + n) * H1 : nullptr, h2);
    if (actor) {
        int a;
        float lp_sel;
        ts_draw(P, h2, u[(size_t)nc * A + y], a, lp_sel);
        if (on) {
            act[(size_t)y * N + n] = a;
            f[(size_t)y * 3 * N + n] = lp_sel;
            act8[(size_t)n * A + y] = (int8_t)a;
        }
    } else {
        // rs_cnn_head_kernel<1>: the state value, to its owner's row or (global critic) to every agent's
        const eh_cmem_t w3 = eh_cmem(P.w3), b3 = eh_cmem(P.b3);
        float v = b3[0];
#pragma unroll
        for (int k = 0; k < H2; ++k) v = __builtin_fmaf(w3[k], h2[k], v);
        if (on) {
            if (C == 1) for (int a = 0; a < A; ++a) f[((size_t)a * 3 + slot) * N + n] = v;
            else f[((size_t)(y - A) * 3 + slot) * N + n] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// rs_cnn_sized_team_step_head: the heads of a team's TRAINING round at a run-time depth flat = 16 p p (the tiled trunk's maps of any
// side; 85 264 at 147 x 147), in two launches.  The walls-off workload is 512 envs: rs_cnn_sized_team_eval_head's grid of 64-image tiles
// would be 8 workgroups per row on 256 CUs, each walking the whole depth.  So the first layer is split over k as well.
//
// Stage 1 (sk_first_layer_kernel), grid = (64-env tiles, k slices, rows): a workgroup takes slice s = floats [SK_SLICE s, SK_SLICE (s + 1))
// of k, cut at flat (the last slice is shorter, a multiple of 16 floats).  Its four waves own the slice's quarters
// [SK_QUARTER w, SK_QUARTER (w + 1)), cut at the slice's end -- a wave's share is a multiple of 16 floats, whole 32-float pieces and
// possibly a tail of 16 (floats 0..7 on the lower lane half, 8..15 on the upper); a wave behind the end adds nothing.  The pieces go
// through eh_step two in flight as in the kernels above; the four partial sums meet in LDS (ts_meet) and are added in wave order; the
// workgroup's 64 x 32 sums go to scratch [row][S][N][32] as float4s.  S = ceil(flat / SK_SLICE) depends on flat alone, so the terms of
// an env's sum and their order depend on neither N nor the grid.  A workgroup whose 64 envs are all masked out returns before the k loop.
//
// Stage 2 (sk_heads_kernel), grid = (64-env tiles, rows), one env per lane: wave w adds the S partial sums of neurons 8 w .. 8 w + 7 in
// slice order, then the bias; wave 0 then runs ts_hidden's / ts_draw's arithmetic (rs_cnn_head's, operation for operation) and writes
// rs_cnn_team_step_head_kernel's outputs.  A masked-out env reads no scratch and writes nothing: the scratch of a masked-in env was
// written by stage 1 in the same call (its tile had that env on).
//
// SK_SLICE: see DESIGN.md section 3 for the lengths tried.
#ifndef RS_SK_SLICE
#define RS_SK_SLICE 4096                            // (-DRS_SK_SLICE=n: an A/B build for scripts/time_cnn_sized_team_collect.py)
#endif
constexpr int SK_SLICE = RS_SK_SLICE;               // floats of k per stage-1 workgroup
constexpr int SK_QUARTER = SK_SLICE / EH_WAVES;     // 1024 per wave: 32 pieces of 32 floats
static_assert(SK_SLICE % 128 == 0 && SK_QUARTER % 32 == 0, "whole pieces per wave in a full slice");

struct SkRows {
    const float* w1[2 * RS_MAX_AGENTS];             // the launched rows' first-layer weights [32][flat]
    const float* a2[2 * RS_MAX_AGENTS];             // and their trunk outputs [N][flat]
};

__global__ void __launch_bounds__(EH_NT) sk_first_layer_kernel(SkRows rows, int flat, const uint8_t* __restrict__ mask,
                                                               float* __restrict__ scratch, int N) {
    __shared__ __align__(16) float part[EH_WAVES][EH_TILE][EH_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int y = blockIdx.z, sl = blockIdx.y, S = gridDim.y;
    const int n0 = blockIdx.x * EH_TILE;
    {   // every wave looks at the same 64 flags, so the four of them agree: nothing to do for this tile -> all leave before the barrier
        const int n = n0 + lane;
        const bool on = n < N && (mask == nullptr || mask[n] != 0);
        if (!__any(on)) return;
    }
    const int len = min(SK_SLICE, flat - sl * SK_SLICE);                        // the slice's floats: a multiple of 16
    const int lw = max(0, min(SK_QUARTER, len - wave * SK_QUARTER));            // the wave's: a multiple of 16
    const int np = lw / 32, tail = lw - 32 * np;                                // tail: 0 or 16
    const size_t k0 = (size_t)sl * SK_SLICE + (size_t)wave * SK_QUARTER;
    // rows past the last image read the last image's (their sums are dropped)
    const int na = n0 + r < N ? n0 + r : N - 1, nb = n0 + 32 + r < N ? n0 + 32 + r : N - 1;
    const float* wp = rows.w1[y] + (size_t)r * flat + k0;
    const float* xa = rows.a2[y] + (size_t)na * flat + k0;
    const float* xb = rows.a2[y] + (size_t)nb * flat + k0;
    v16f acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
    struct Piece { float4 w[4], a[4], b[4]; };
    auto fetch = [&](Piece& q, int g) {                               // the lane half's 16 floats of piece g
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = 32 * g + 16 * h + 4 * i;
            q.w[i] = *reinterpret_cast<const float4*>(wp + o);
            q.a[i] = *reinterpret_cast<const float4*>(xa + o);
            q.b[i] = *reinterpret_cast<const float4*>(xb + o);
        }
    };
    auto consume = [&](const Piece& q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) eh_step(acc0, acc1, q.w[i], q.a[i], q.b[i]);
    };
    if (np > 0) {                                                     // (np is wave-uniform)
        Piece p0, p1;
        fetch(p0, 0);
        fetch(p1, np > 1 ? 1 : 0);                                    // (a single piece is requested twice; the copy is dropped)
        int g = 0;
#pragma unroll 1
        for (; g + 2 < np; g += 2) {                                  // p0 holds piece g, p1 piece g + 1, both with a successor
            consume(p0);
            __builtin_amdgcn_sched_barrier(0);
            fetch(p0, g + 2);
            __builtin_amdgcn_sched_barrier(0);
            consume(p1);
            __builtin_amdgcn_sched_barrier(0);
            fetch(p1, g + 3 < np ? g + 3 : np - 1);                   // (an odd np re-requests its last piece; it is dropped)
            __builtin_amdgcn_sched_barrier(0);
        }
        consume(p0);                                                  // the last two pieces, or the last one
        if (g + 1 < np) consume(p1);
    }
    if (tail == 16) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = 32 * np + 8 * h + 4 * i;
            eh_step(acc0, acc1, *reinterpret_cast<const float4*>(wp + o), *reinterpret_cast<const float4*>(xa + o),
                    *reinterpret_cast<const float4*>(xb + o));
        }
    }
    ts_meet(part, acc0, acc1);
    // thread -> (env tid / 4, neurons 8 (tid % 4) .. + 7): the four quarters in wave order, two float4 stores
    const int e = tid >> 2, j0 = 8 * (tid & 3);
    if (n0 + e < N) {
        float* dst = scratch + (((size_t)y * S + sl) * N + n0 + e) * H1 + j0;
#pragma unroll
        for (int k = 0; k < 8; k += 4) {
            float4 s = *reinterpret_cast<const float4*>(&part[0][e][j0 + k]);
#pragma unroll
            for (int w = 1; w < EH_WAVES; ++w) {
                const float4 q = *reinterpret_cast<const float4*>(&part[w][e][j0 + k]);
                s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
            }
            *reinterpret_cast<float4*>(dst + k) = s;
        }
    }
}

__global__ void __launch_bounds__(EH_NT) sk_heads_kernel(TsNets nets, int A, int C, int row0, int slot, int S,
                                                         const float* __restrict__ scratch, const float* __restrict__ u,
                                                         int64_t* __restrict__ act, float* __restrict__ f, int8_t* __restrict__ act8,
                                                         const uint8_t* __restrict__ mask, float* __restrict__ y1_out, int N) {
    __shared__ __align__(16) float y1s[EH_TILE][EH_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int y = row0 + blockIdx.y;                                  // the network; blockIdx.y is its row of the scratch
    const int n = blockIdx.x * EH_TILE + lane;
    const bool on = n < N && (mask == nullptr || mask[n] != 0);
    if (!__any(on)) return;                                           // the four waves agree (the same 64 flags)
    const rs_cnn_head_params P = nets.net[y];
    {   // wave w: neurons 8 w .. 8 w + 7 of the lane's env, the slices in order 0 .. S - 1, then the bias
        const int j0 = 8 * wave;
        float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
        if (on) {
            const float* src = scratch + (((size_t)blockIdx.y * S) * N + n) * H1 + j0;
            const size_t stride = (size_t)N * H1;
            s0 = *reinterpret_cast<const float4*>(src);
            s1 = *reinterpret_cast<const float4*>(src + 4);
#pragma unroll 8
            for (int sl = 1; sl < S; ++sl) {
                const float4 q0 = *reinterpret_cast<const float4*>(src + sl * stride);
                const float4 q1 = *reinterpret_cast<const float4*>(src + sl * stride + 4);
                s0.x += q0.x; s0.y += q0.y; s0.z += q0.z; s0.w += q0.w;
                s1.x += q1.x; s1.y += q1.y; s1.z += q1.z; s1.w += q1.w;
            }
        }
        const eh_cmem_t b1 = eh_cmem(P.b1);
        s0.x += b1[j0]; s0.y += b1[j0 + 1]; s0.z += b1[j0 + 2]; s0.w += b1[j0 + 3];
        s1.x += b1[j0 + 4]; s1.y += b1[j0 + 5]; s1.z += b1[j0 + 6]; s1.w += b1[j0 + 7];
        if (y1_out && on) {
            float* dst = y1_out + ((size_t)y * N + n) * H1 + j0;
            *reinterpret_cast<float4*>(dst) = s0;
            *reinterpret_cast<float4*>(dst + 4) = s1;
        }
        *reinterpret_cast<float4*>(&y1s[lane][j0]) = s0;
        *reinterpret_cast<float4*>(&y1s[lane][j0 + 4]) = s1;
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- behind y1: ReLU, then csrc/rs_cnn_head.hpp's layers
    float h1[H1], h2[H2];
#pragma unroll
    for (int k = 0; k < H1; k += 4) {
        const float4 s = *reinterpret_cast<const float4*>(&y1s[lane][k]);
        h1[k] = fmaxf(s.x, 0.0f); h1[k + 1] = fmaxf(s.y, 0.0f); h1[k + 2] = fmaxf(s.z, 0.0f); h1[k + 3] = fmaxf(s.w, 0.0f);
    }
    rs_cnn_head_layer2(P.w2, P.b2, h1, h2);
    const int nc = n < N ? n : N - 1;
    if (y < A) {
        int a;
        float lp_sel;
        rs_cnn_head_draw(P.w3, P.b3, h2, u[(size_t)nc * A + y], a, lp_sel);
        if (on) {
            act[(size_t)y * N + n] = a;
            f[(size_t)y * 3 * N + n] = lp_sel;
            act8[(size_t)n * A + y] = (int8_t)a;
        }
    } else {
        // the state value, to its owner's row or (global critic) to every agent's
        const float v = rs_cnn_head_value(P.w3, P.b3, h2);
        if (on) {
            if (C == 1) for (int a = 0; a < A; ++a) f[((size_t)a * 3 + slot) * N + n] = v;
            else f[((size_t)(y - A) * 3 + slot) * N + n] = v;
        }
    }
}

inline int sk_depth_ok(int32_t flat) {
    int p = 4;
    while (p < 128 && 16 * p * p < flat) ++p;
    return 16 * p * p == flat;                                        // the tiled trunk's output: 16 p p, p = 4..128
}

}  // namespace

extern "C" {

int32_t rs_cnn_sized_team_head_slice_floats(void) { return SK_SLICE; }

int64_t rs_cnn_sized_team_head_scratch_floats(int32_t flat, int32_t num_rows, int32_t num_envs) {
    if (!sk_depth_ok(flat) || num_rows < 1 || num_envs < 1) return 0;
    return (int64_t)num_rows * ((flat + SK_SLICE - 1) / SK_SLICE) * num_envs * H1;
}

int rs_cnn_sized_team_step_head(const rs_cnn_head_params* actors, int32_t num_agents, const rs_cnn_head_params* critics,
                                int32_t num_critics, int32_t flat, const float* a2_actor, const float* a2_critic, const float* u,
                                int64_t* act, float* logp_val_boot, int8_t* act8, const uint8_t* mask, float* y1_out, float* scratch,
                                int64_t scratch_floats, int32_t num_envs, rs_stream_t stream) {
    const bool step = u != nullptr;
    if (num_agents < 1 || num_agents > RS_MAX_AGENTS || (num_critics != 1 && num_critics != num_agents) || num_envs < 1) return RS_ERR_INVALID_ARG;
    if (!critics || !a2_critic || !logp_val_boot) return RS_ERR_INVALID_ARG;
    if (step ? (!actors || !a2_actor || !act || !act8) : !mask) return RS_ERR_INVALID_ARG;
    auto whole = [](const rs_cnn_head_params& p) { return p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3; };
    for (int c = 0; c < num_critics; ++c)
        if (!whole(critics[c])) return RS_ERR_INVALID_ARG;
    for (int a = 0; step && a < num_agents; ++a)
        if (!whole(actors[a])) return RS_ERR_INVALID_ARG;
    const int rows = step ? num_agents + num_critics : num_critics;                              // the bootstrap round: the critic rows alone
    if (!sk_depth_ok(flat) || !scratch || scratch_floats < rs_cnn_sized_team_head_scratch_floats(flat, rows, num_envs)) return RS_ERR_INVALID_ARG;
    const int row0 = step ? 0 : (int)num_agents;
    TsNets nets;
    for (int i = 0; i < 2 * RS_MAX_AGENTS; ++i) nets.net[i] = critics[0];                       // the slots no row reads
    for (int a = 0; step && a < num_agents; ++a) nets.net[a] = actors[a];
    for (int c = 0; c < num_critics; ++c) nets.net[num_agents + c] = critics[c];
    SkRows rw;
    for (int i = 0; i < 2 * RS_MAX_AGENTS; ++i) {                                               // launched row i is network row0 + i
        const int y = row0 + (i < rows ? i : 0);
        rw.w1[i] = nets.net[y].w1;
        rw.a2[i] = y < num_agents ? a2_actor + (size_t)y * num_envs * flat : a2_critic + (size_t)(y - num_agents) * num_envs * flat;
    }
    const int tiles = (num_envs + EH_TILE - 1) / EH_TILE, S = (flat + SK_SLICE - 1) / SK_SLICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sk_first_layer_kernel, dim3(tiles, S, rows), dim3(EH_NT), 0, s, rw, (int)flat, mask, scratch, (int)num_envs);
    hipLaunchKernelGGL(sk_heads_kernel, dim3(tiles, rows), dim3(EH_NT), 0, s, nets, (int)num_agents, (int)num_critics, row0, step ? 1 : 2, S,
                       (const float*)scratch, u, act, logp_val_boot, act8, mask, y1_out, (int)num_envs);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_team_eval_head(const rs_cnn_head_params* heads, int32_t num_agents, const float* a2, const float* u, const uint8_t* alive,
                          int8_t* act8, int64_t* act, float* logp, float* y1_out, int32_t num_envs, rs_stream_t stream) {
    if (!heads || !a2 || !u || !alive || !act8 || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_envs < 1) return RS_ERR_INVALID_ARG;
    for (int a = 0; a < num_agents; ++a)
        if (!heads[a].w1 || !heads[a].b1 || !heads[a].w2 || !heads[a].b2 || !heads[a].w3 || !heads[a].b3) return RS_ERR_INVALID_ARG;
    EhNets nets;
    for (int a = 0; a < RS_MAX_AGENTS; ++a) nets.head[a] = heads[a < num_agents ? a : 0];     // the slots behind the team repeat agent 0 (never read)
    hipLaunchKernelGGL(rs_cnn_team_eval_head_kernel, dim3((num_envs + EH_TILE - 1) / EH_TILE, num_agents), dim3(EH_NT), 0,
                       static_cast<hipStream_t>(stream), nets, (int)num_agents, a2, u, alive, act8, act, logp, y1_out, (int)num_envs);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_sized_team_eval_head(const rs_cnn_head_params* heads, int32_t num_agents, int32_t flat, const float* a2, const float* u,
                                const uint8_t* alive, int8_t* act8, int64_t* act, float* logp, float* y1_out, int32_t num_envs,
                                rs_stream_t stream) {
    if (!heads || !a2 || !u || !alive || !act8 || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_envs < 1) return RS_ERR_INVALID_ARG;
    for (int a = 0; a < num_agents; ++a)
        if (!heads[a].w1 || !heads[a].b1 || !heads[a].w2 || !heads[a].b2 || !heads[a].w3 || !heads[a].b3) return RS_ERR_INVALID_ARG;
    int p = 4;
    while (p < 128 && 16 * p * p < flat) ++p;
    if (16 * p * p != flat) return RS_ERR_INVALID_ARG;                // the tiled trunk's output: 16 p p, p = 4..128
    EhNets nets;
    for (int a = 0; a < RS_MAX_AGENTS; ++a) nets.head[a] = heads[a < num_agents ? a : 0];     // the slots behind the team repeat agent 0 (never read)
    hipLaunchKernelGGL(rs_cnn_sized_team_eval_head_kernel, dim3((num_envs + EH_TILE - 1) / EH_TILE, num_agents), dim3(EH_NT), 0,
                       static_cast<hipStream_t>(stream), nets, (int)num_agents, (int)flat, a2, u, alive, act8, act, logp, y1_out, (int)num_envs);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_team_step_head(const rs_cnn_head_params* actors, int32_t num_agents, const rs_cnn_head_params* critics, int32_t num_critics,
                          const float* a2_actor, const float* a2_critic, const float* u, int64_t* act, float* logp_val_boot, int8_t* act8,
                          const uint8_t* mask, float* y1_out, int32_t num_envs, rs_stream_t stream) {
    const bool step = u != nullptr;
    if (num_agents < 1 || num_agents > RS_MAX_AGENTS || (num_critics != 1 && num_critics != num_agents) || num_envs < 1) return RS_ERR_INVALID_ARG;
    if (!critics || !a2_critic || !logp_val_boot) return RS_ERR_INVALID_ARG;
    if (step ? (!actors || !a2_actor || !act || !act8) : !mask) return RS_ERR_INVALID_ARG;
    auto whole = [](const rs_cnn_head_params& p) { return p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3; };
    for (int c = 0; c < num_critics; ++c)
        if (!whole(critics[c])) return RS_ERR_INVALID_ARG;
    for (int a = 0; step && a < num_agents; ++a)
        if (!whole(actors[a])) return RS_ERR_INVALID_ARG;
    TsNets nets;
    for (int i = 0; i < 2 * RS_MAX_AGENTS; ++i) nets.net[i] = critics[0];                       // the slots no row reads
    for (int a = 0; step && a < num_agents; ++a) nets.net[a] = actors[a];
    for (int c = 0; c < num_critics; ++c) nets.net[num_agents + c] = critics[c];
    const int rows = step ? num_agents + num_critics : num_critics;                              // the bootstrap round: the critic rows alone
    hipLaunchKernelGGL(rs_cnn_team_step_head_kernel, dim3((num_envs + EH_TILE - 1) / EH_TILE, rows), dim3(EH_NT), 0,
                       static_cast<hipStream_t>(stream), nets, (int)num_agents, (int)num_critics, step ? 0 : (int)num_agents, step ? 1 : 2,
                       a2_actor, a2_critic, u, act, logp_val_boot, act8, mask, y1_out, (int)num_envs);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

// rs_pfgru_sized_train.hip -- K13's contract (csrc/rs_pfgru_train.hip: loss and parameter gradients of the PFGRU location predictor over
// whole episodes, a forward-walk launch and a backward-walk launch per pass of update_model) at hidden widths H = 8, 16, .., 64, the
// width a template parameter.  40 particles, 3 inputs, alpha from the caller, tanh and hid_obs = Linear(H, 24)-ReLU-Linear(24, 2)-ReLU as
// the reference fixes them; the loss is the one of include/radsearch.h (rs_pfgru_train); resampling indices are constants of the backward
// pass, as in autograd.  The pass's draws as buffers: rs_pfgru_sized_draws (rs_draws.hip).
//
// Built for correctness first: none of K13's tuning (one wave per episode, 24 units in registers, matrix cores, scalar weight streams)
// carries to 64 units, where the weight-gradient accumulators alone are 17.4 k floats per episode.
//
// Decomposition, the same at every width: ONE 256-thread workgroup (four waves) per episode in both walks.  What belongs to a particle
// lives in LDS arrays of 40 rows; every product is a loop nest over (output, particle) items spread over the 256 threads, every sum over
// a set's 40 particles runs in index order in one thread, and workgroup barriers separate the phases of a step.  No atomics: an episode's
// slab row and loss depend on that episode alone and two launches return the same bits.
//   forward walk   per step: [z | r] = sigmoid(W_zr [h0, x] + b), [mu | var] = W_n [r h0, x] + b (thread = one output column x five
//                  particles, weights k-major from global memory, the particles' inputs from LDS), candidate / h1 element-wise, the
//                  observation logit and both log-softmaxes by the particle's own thread, the float64 CDF and its search as K11s, the
//                  gather; it stores the step's gates z | r | n | eps * softplus'(var), both log-weight vectors, the indices (when it
//                  picked them) and the resampled set.
//   backward walk  per step: hid_obs forward on the 40 resampled particles and their weighted mean, the loss terms and d loss / d out,
//                  hid_obs backwards, the softmax / resampling derivatives, the gather backwards (every source particle sums its
//                  takers' rows in index order), the gates backwards, and the three transposed products (thread = one input unit x five
//                  particles, weights in their native [out][in] layout).  The weight gradients are sums over particles of outer products:
//                  each thread owns a share of every gradient matrix IN REGISTERS for the whole episode -- rows ty + 16 i x columns
//                  tx + 16 j of d[fc_z | fc_r] and d fc_n ((H / 8) x ceil((H + 4) / 16) accumulators each: 2 x 40 at 64 units), strided
//                  elements of the thin ones -- and contracts over the 40 particles with FMAs on operands staged in LDS.
//
// Resources per width (gfx950; the bounds are held by tests/test_pfgru_sized_train_resources.py; no scratch and no spill at any width).
// A workgroup is one wave on each SIMD of its CU, so workgroups per CU = waves per SIMD = min(512 / VGPRs, 160 KB / LDS):
//   H     forward walk: VGPRs, LDS      backward walk: VGPRs, LDS      waves per SIMD forward / backward
//   8     <= 128,  9.3 KB               <= 128, 21.4 KB                4 / 4
//   16    <= 128, 16.8 KB               <= 128, 31.5 KB                4 / 4
//   24    <= 128, 24.3 KB               <= 128, 39.0 KB                4 / 4
//   32    <= 128, 31.8 KB               <= 168, 49.1 KB                4 / 3
//   40    <= 128, 39.3 KB               <= 168, 56.6 KB                4 / 2 (LDS)
//   48    <= 128, 46.8 KB               <= 256, 66.6 KB                3 / 2 (LDS forward)
//   56    <= 128, 54.3 KB               <= 256, 74.1 KB                2 / 2 (LDS forward)
//   64    <= 128, 61.8 KB               <= 256, 84.2 KB                2 / 1 (LDS)
// The inner loops over particles / units are unrolled by 2-8 only: fully unrolled, hipcc hoists every LDS read of a 40-particle loop in
// front of its FMAs and spills (up to 2.1 KB of scratch per lane at 40 units).
//
// Packed weights (floats; packer: rada2c.py: pack_sized_train_weights), K = H + 3 inputs [h | x], R = 2 H gate rows:
//   ZRT [K][R] k-major [fc_z | fc_r] | ZRB [R] | NT [K][R] k-major fc_n | NB [R] | ZR [R][K] | N [R][K] | O [K] | OB [1] |
//   H0T [H][24] k-major hid_obs.0 | H0B [24] | H0 [24][H] | H2 [2][24] | H2B [2] | pad to a multiple of 16
// Gradient slab (floats): d[fc_z | fc_r] [R][H + 4] (column H + 3 = bias) | d fc_n [R][H + 4] | d hid_obs.0 [24][H + 1] |
//   d hid_obs.2 [2][25] | d fc_obs [H + 4] | pad to a multiple of 16
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_draws.hpp"

namespace {

constexpr int P = RS_PFGRU_PARTICLES, IN = 3, NT = 256, PG = 5, NPG = P / PG;      // 40 particles in 8 groups of 5
__host__ __device__ constexpr int r16(int v) { return (v + 15) / 16 * 16; }
bool width_ok(int H) { return H >= 8 && H <= 64 && H % 8 == 0; }

struct WLayout {
    int ZRT, ZRB, NT_, NB, ZR, N, O, OB, H0T, H0B, H0, H2, H2B, stride;
};
__host__ __device__ constexpr WLayout wlayout(int H) {
    const int K = H + IN, R = 2 * H;
    const int ZRT = 0, ZRB = ZRT + K * R, NT_ = ZRB + R, NB = NT_ + K * R, ZR = NB + R, N = ZR + R * K, O = N + R * K, OB = O + K,
              H0T = OB + 1, H0B = H0T + H * 24, H0 = H0B + 24, H2 = H0 + 24 * H, H2B = H2 + 48;
    return WLayout{ZRT, ZRB, NT_, NB, ZR, N, O, OB, H0T, H0B, H0, H2, H2B, r16(H2B + 2)};
}
struct GLayout {
    int ZR, N, H0, H2, O, end, stride;
};
__host__ __device__ constexpr GLayout glayout(int H) {
    const int R = 2 * H, C = H + 4;
    const int ZR = 0, N = ZR + R * C, H0 = N + R * C, H2 = H0 + 24 * (H + 1), O = H2 + 50, end = O + C;
    return GLayout{ZR, N, H0, H2, O, end, r16(end)};
}

// the hardware transcendentals as K11s / K13 (rs_draws.hpp); the float64 CDF quotient stays IEEE
__device__ __forceinline__ float st_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
// rolled, one value per read: the backward walk's rows (s.ve1 + Q, Q = 41) are not 16-byte aligned as rs_max40 / rs_sum40 need them
__device__ __forceinline__ float st_max40(const float* v) {
    float m = -INFINITY;
#pragma unroll 8
    for (int i = 0; i < P; ++i) m = fmaxf(m, v[i]);
    return m;
}
__device__ __forceinline__ float st_sum40(const float* v) {           // index order
    float s = 0.0f;
#pragma unroll 8
    for (int i = 0; i < P; ++i) s += v[i];
    return s;
}

struct StArgs {
    const float* w;           // [wlayout(H).stride]
    const float* obs;         // [L][E][11] (columns 0..2 feed the PFGRU)
    const float* tar;         // [L][E][2]
    const float* bp;          // [L][E]
    const int64_t* lens;      // [E]
    const float* w_ep;        // [E]
    const float* h0;          // [E][P][H]
    const float* eps;         // [L][E][P][H]
    const double* u;          // [L][E][P] or NULL: idx[] holds the indices to take
    float* hs;                // [L][E][P][H]     scratch: the resampled particle set after every step
    float* ps;                // [L][E][2][P]     scratch: log weights before (row 0) and after (row 1) the step's resampling
    float* gates;             // [L][E][4][P][H]  scratch: z | r | n | eps * softplus'(var)
    int32_t* idx;             // [L][E][P]
    float* loss;              // [E]
    float* grads;             // [E][glayout(H).stride]
    int L, E;
    float alpha, floor_, l2w, l1w, elbo;
};

// out[p][o] = b[o] + sum_k Wt[k][o] in[p][k] (k < H from the LDS rows `in`, then the three inputs x) for one output column o and the five
// particles of group pg
template <int H>
__device__ __forceinline__ void fw_product(const float* Wt, const float* b, const float* in, int IS, const float (&x)[IN], int o, int pg,
                                           float (&acc)[PG]) {
    constexpr int R = 2 * H;
    const float b0 = b[o];
#pragma unroll
    for (int j = 0; j < PG; ++j) acc[j] = b0;
    const float* row = in + pg * PG * IS;
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
        const float w = Wt[k * R + o];
#pragma unroll
        for (int j = 0; j < PG; ++j) acc[j] = fmaf(w, row[j * IS + k], acc[j]);
    }
#pragma unroll
    for (int k = 0; k < IN; ++k) {
        const float w = Wt[(H + k) * R + o];
#pragma unroll
        for (int j = 0; j < PG; ++j) acc[j] = fmaf(w, x[k], acc[j]);
    }
}

template <int H>
__global__ void __launch_bounds__(NT, 2) rs_pfgru_sized_train_fwd_kernel(StArgs a_) {
    constexpr int R = 2 * H, HS = H + 1, AS = R + 1;
    constexpr WLayout W = wlayout(H);
    __shared__ __align__(16) float hin[P * HS];                       // the step's input particles
    __shared__ __align__(16) float rh[P * HS];                        // r * h0
    __shared__ __align__(16) float zz[P * HS];                        // z
    __shared__ __align__(16) float h1s[P * HS];                       // h1 (the gather's source)
    __shared__ __align__(16) float an[P * AS];                        // [mu | var]
    __shared__ __align__(16) double cdf[P];
    __shared__ float va[P], vb[P], vc[P];
    __shared__ int vidx[P];
    const int tid = threadIdx.x;
    const int e = blockIdx.x;
    const int E = a_.E;
    const int len = min(max((int)a_.lens[e], 0), a_.L);
    const float al = a_.alpha, floor_ = a_.floor_;
    const size_t PH = (size_t)P * H;
    for (int i = tid; i < P * H; i += NT) hin[(i / H) * HS + i % H] = a_.h0[(size_t)e * PH + i];
    float p0 = RS_LOG_INV_P;                                         // thread q < 40 carries particle q's log weight
    __syncthreads();
    for (int t = 0; t < len; ++t) {
        const size_t te = (size_t)t * E + e;
        // the weights do not change from step to step: the pointer re-enters every step, or their loads are hoisted out of the
        // episode loop into registers that do not exist (scratch)
        const float* w = a_.w;
        asm volatile("" : "+s"(w));
        float x[IN];
#pragma unroll
        for (int k = 0; k < IN; ++k) x[k] = a_.obs[te * RS_OBS_DIM + k];
        float* gz = a_.gates + te * 4 * PH;
        // ---- z, r
        for (int it = tid; it < NPG * R; it += NT) {
            const int o = it % R, pg = it / R;
            float acc[PG];
            fw_product<H>(w + W.ZRT, w + W.ZRB, hin, HS, x, o, pg, acc);
#pragma unroll
            for (int j = 0; j < PG; ++j) {
                const int p = pg * PG + j;
                const float s = rs_sigmoid(acc[j]);
                if (o < H) {
                    zz[p * HS + o] = s;
                    gz[(size_t)p * H + o] = s;
                } else {
                    rh[p * HS + o - H] = s * hin[p * HS + o - H];
                    gz[PH + (size_t)p * H + o - H] = s;
                }
            }
        }
        __syncthreads();
        // ---- mu, var
        for (int it = tid; it < NPG * R; it += NT) {
            const int o = it % R, pg = it / R;
            float acc[PG];
            fw_product<H>(w + W.NT_, w + W.NB, rh, HS, x, o, pg, acc);
#pragma unroll
            for (int j = 0; j < PG; ++j) an[(pg * PG + j) * AS + o] = acc[j];
        }
        __syncthreads();
        // ---- candidate and h1
        for (int i = tid; i < P * H; i += NT) {
            const int p = i / H, u = i % H;
            const float ep = a_.eps[te * PH + i];
            const float var = an[p * AS + H + u];
            const float ex = __builtin_amdgcn_exp2f(1.44269504f * var);
            const bool big = var > 20.0f;                             // F.softplus: identity (slope 1) beyond 20
            const float sp = big ? var : 0.69314718f * __builtin_amdgcn_logf(1.0f + ex);
            const float es = big ? ep : ep * (1.0f - __builtin_amdgcn_rcpf(1.0f + ex));
            const float y = an[p * AS + u] + ep * sp;
            const float n = rs_tanh(y);
            const float z = zz[p * HS + u];
            h1s[p * HS + u] = (1.0f - z) * n + z * hin[p * HS + u];
            gz[2 * PH + i] = n;
            gz[3 * PH + i] = es;
        }
        __syncthreads();
        // ---- observation likelihood, log-softmax over the particles
        const int q = tid < P ? tid : P - 1;
        float lg = w[W.OB];
#pragma unroll 4
        for (int u = 0; u < H; ++u) lg = fmaf(w[W.O + u], h1s[q * HS + u], lg);
#pragma unroll
        for (int k = 0; k < IN; ++k) lg = fmaf(w[W.O + H + k], x[k], lg);
        lg += p0;
        if (tid < P) va[tid] = lg;
        __syncthreads();
        const float mx = st_max40(va);
        const float e1 = rs_exp(lg - mx);
        if (tid < P) vb[tid] = e1;
        __syncthreads();
        const float p1 = (lg - mx) - rs_log(st_sum40(vb));
        __syncthreads();
        if (tid < P) {
            va[tid] = al * rs_exp(p1) + floor_;
            vc[tid] = p1;
        }
        __syncthreads();
        // ---- soft resampling: float64 inverse CDF of the caller's uniform, or the recorded index
        int idx = 0;
        if (a_.u) {
            double run = 0.0, mine = 0.0;                            // float64 prefix sums in index order
#pragma unroll 4
            for (int i = 0; i < P; ++i) {
                run += (double)va[i];
                mine = (i == q) ? run : mine;
            }
            if (tid < P) cdf[tid] = mine / run;
            __syncthreads();                                         // (a_.u is a launch argument: every thread takes this branch or none)
            const double ru = a_.u[te * P + q];
#pragma unroll 4
            for (int j = 0; j < P; ++j) idx += (cdf[j] <= ru) ? 1 : 0;      // searchsorted(..., right=True)
            idx = min(idx, P - 1);
        } else {
            idx = min(max(a_.idx[te * P + q], 0), P - 1);
        }
        float pn = rs_exp(vc[idx]);
        pn = rs_log(st_div(pn, al * pn + floor_));
        if (tid < P) {
            vb[tid] = pn;
            vidx[tid] = idx;
        }
        __syncthreads();
        const float mx2 = st_max40(vb);
        const float e2 = rs_exp(pn - mx2);
        __syncthreads();
        if (tid < P) va[tid] = e2;
        __syncthreads();
        p0 = pn - (rs_log(st_sum40(va)) + mx2);
        if (tid < P) {
            a_.ps[te * 2 * P + tid] = p1;
            a_.ps[te * 2 * P + P + tid] = p0;
            if (a_.u) a_.idx[te * P + tid] = idx;
        }
        // ---- the gather: the resampled set is the next step's input and what the backward walk reads
        for (int i = tid; i < P * H; i += NT) {
            const int p = i / H, u = i % H;
            const float v = h1s[vidx[p] * HS + u];
            hin[p * HS + u] = v;
            a_.hs[te * PH + i] = v;
        }
        __syncthreads();
    }
}

// out[p][k] = sum over o < R of Wn[o][k] d[p][o] (native [R][K] weights, d rows in LDS) for one input unit k and the five particles of pg
template <int H>
__device__ __forceinline__ void bw_product(const float* Wn, const float* d, int DS, int k, int pg, float (&acc)[PG]) {
    constexpr int R = 2 * H, K = H + IN;
#pragma unroll
    for (int j = 0; j < PG; ++j) acc[j] = 0.0f;
    const float* row = d + pg * PG * DS;
#pragma unroll 4
    for (int o = 0; o < R; ++o) {
        const float w = Wn[o * K + k];
#pragma unroll
        for (int j = 0; j < PG; ++j) acc[j] = fmaf(w, row[j * DS + o], acc[j]);
    }
}

// acc[i][j] += sum over the 40 particles of D[p][ty + 16 i] * I[p][tx + 16 j]
template <int RI, int CJ>
__device__ __forceinline__ void outer_acc(const float* D, int DS, const float* I, int IS, int ty, int tx, float (&acc)[RI][CJ]) {
#pragma unroll 2
    for (int p = 0; p < P; ++p) {
        float dv[RI], iv[CJ];
#pragma unroll
        for (int i = 0; i < RI; ++i) dv[i] = D[p * DS + ty + 16 * i];
#pragma unroll
        for (int j = 0; j < CJ; ++j) iv[j] = I[p * IS + tx + 16 * j];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int j = 0; j < CJ; ++j) acc[i][j] = fmaf(dv[i], iv[j], acc[i][j]);
    }
}

template <int H>
struct BwLds {
    static constexpr int R = 2 * H, HS = H + 1, DS = R + 1, C = H + 4, CP = r16(C), IS = CP + 1, RS = H + 2, Q = P + 1;
    float D[P * DS];          // the gate-gradient rows of an outer / transposed product; before that hid_obs' d loss / d input [41][HS]
    float I[Q * IS];          // the input rows [v | 1] of an outer product (41 rows: the particles and their weighted mean)
    float dh[P * HS];         // d loss / d (the step's resampled set) from the steps behind it
    float dhr[P * RS];        // the same with this step's terms, column H = d loss / d (log weight); later h1
    float dh1[P * HS];        // after the gather backwards; later d z
    float t1[P * HS];         // d (r h0)
    float uu[Q * 25], du[Q * 25];
    float out[Q * 2], dop[Q * 2];
    float ve2[2 * Q], ve1[2 * Q];
    float pi[P], vp1[P], vtmp[P], vdp1[P], vdlp[P];
    int vidx[P];
};

template <int H>
__global__ void __launch_bounds__(NT, H <= 56 ? 2 : 1) rs_pfgru_sized_train_bwd_kernel(StArgs a_) {
    using S = BwLds<H>;
    constexpr int R = S::R, HS = S::HS, DS = S::DS, C = S::C, IS = S::IS, RS = S::RS, Q = S::Q;
    constexpr int RI = R / 16, CJ = S::CP / 16;                      // a thread's share of d[fc_z | fc_r] and d fc_n: rows ty + 16 i, columns tx + 16 j
    constexpr int NH0 = (24 * HS + NT - 1) / NT;                     // ... and of d hid_obs.0: elements tid + 256 j
    constexpr WLayout W = wlayout(H);
    constexpr GLayout G_ = glayout(H);
    static_assert(Q * HS <= P * DS, "hid_obs' input gradient fits the gate-gradient rows");
    __shared__ __align__(16) S s;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int e = blockIdx.x;
    const int E = a_.E;
    const int len = min(max((int)a_.lens[e], 0), a_.L);
    const float G = a_.w_ep[e];
    float* g = a_.grads + (size_t)e * G_.stride;
    if (G == 0.0f || len == 0) {                                     // an episode without weight: an exactly zero row and loss
        for (int i = tid; i < G_.stride; i += NT) g[i] = 0.0f;
        if (tid == 0) a_.loss[e] = 0.0f;
        return;
    }
    const float al = a_.alpha, floor_ = a_.floor_;
    const float l2w = a_.l2w, l1w = a_.l1w, elbo = a_.elbo;
    const float inv_nel = 1.0f / (float)(2 * len);
    const size_t PH = (size_t)P * H;
    {
        float* z = reinterpret_cast<float*>(&s);
        for (int i = tid; i < (int)(sizeof(S) / sizeof(float)); i += NT) z[i] = 0.0f;      // dh = 0; the padding columns of I stay 0
    }
    float accZR[RI][CJ], accN[RI][CJ], accH0[NH0], accH2 = 0.0f, accO = 0.0f;
#pragma unroll
    for (int i = 0; i < RI; ++i)
#pragma unroll
        for (int j = 0; j < CJ; ++j) { accZR[i][j] = 0.0f; accN[i][j] = 0.0f; }
#pragma unroll
    for (int j = 0; j < NH0; ++j) accH0[j] = 0.0f;
    float dp = 0.0f;                                                 // thread q < 40: d loss / d (particle q's log weight after the step)
    float l2s = 0.0f, l1s = 0.0f, l2ps = 0.0f, l1ps = 0.0f;          // the episode's four loss terms (thread 40)
    const int q = tid < P ? tid : P - 1;
    __syncthreads();

    for (int t = len - 1; t >= 0; --t) {
        const size_t te = (size_t)t * E + e;
        const float* w = a_.w;                                       // (re-enters every step: see the forward walk)
        asm volatile("" : "+s"(w));
        const float* hprev = t > 0 ? a_.hs + (te - E) * PH : a_.h0 + (size_t)e * PH;      // the step's input particles
        const float* gz = a_.gates + te * 4 * PH;
        float x[IN];
#pragma unroll
        for (int k = 0; k < IN; ++k) x[k] = a_.obs[te * RS_OBS_DIM + k];
        // ---- the resampled set [v | 1], its log weights, the indices
        if (tid < P) {
            s.vp1[tid] = a_.ps[te * 2 * P + tid];
            s.pi[tid] = rs_exp(a_.ps[te * 2 * P + P + tid]);
            s.vidx[tid] = min(max(a_.idx[te * P + tid], 0), P - 1);
        }
        for (int i = tid; i < P * H; i += NT) s.I[(i / H) * IS + i % H] = a_.hs[te * PH + i];
        if (tid < Q) s.I[tid * IS + H] = 1.0f;
        __syncthreads();
        // ---- weighted mean of the resampled particles (row 40)
        if (tid < H) {
            float mean = 0.0f;
#pragma unroll 4
            for (int p = 0; p < P; ++p) mean += s.pi[p] * s.I[p * IS + tid];
            s.I[P * IS + tid] = mean;
        }
        __syncthreads();
        // ---- hid_obs forward on the 41 rows
        for (int it = tid; it < Q * 24; it += NT) {
            const int row = it / 24, j = it % 24;
            float acc = w[W.H0B + j];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(w[W.H0T + k * 24 + j], s.I[row * IS + k], acc);
            s.uu[row * 25 + j] = fmaxf(acc, 0.0f);
        }
        __syncthreads();
        if (tid < Q * 2) {
            const int row = tid >> 1, c = tid & 1;
            float acc = w[W.H2B + c];
#pragma unroll 4
            for (int j = 0; j < 24; ++j) acc = fmaf(w[W.H2 + c * 24 + j], s.uu[row * 25 + j], acc);
            s.out[tid] = fmaxf(acc, 0.0f);
        }
        __syncthreads();
        // ---- the step's loss terms and d loss / d out
        const float bpt = a_.bp[te];
        const float tr[2] = {a_.tar[te * 2], a_.tar[te * 2 + 1]};
        if (tid < P) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float d = s.out[tid * 2 + c] - tr[c];
                s.ve2[c * Q + tid] = rs_exp(-d * d * bpt);
                s.ve1[c * Q + tid] = rs_exp(-fabsf(d) * bpt);
            }
        }
        __syncthreads();
        if (tid < Q) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float o = s.out[tid * 2 + c];
                const float d = o - tr[c];
                const float y2 = st_sum40(s.ve2 + c * Q) * (1.0f / P);
                float dout;
                if (tid < P) {
                    float gpart = st_div(l2w * 2.0f * d * bpt * s.ve2[c * Q + tid], P * y2);
                    if (l1w != 0.0f) {
                        const float y1 = st_sum40(s.ve1 + c * Q) * (1.0f / P);
                        const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                        gpart += st_div(l1w * 10.0f * sg * bpt * s.ve1[c * Q + tid], P * y1);
                    }
                    dout = G * elbo * gpart * inv_nel;
                } else {                                             // the mean prediction; this thread also keeps the episode's loss sums
                    l2ps += -rs_log(y2);
                    if (l1w != 0.0f) l1ps += -rs_log(st_sum40(s.ve1 + c * Q) * (1.0f / P));
                    const float sgm = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                    l2s += d * d * bpt;
                    l1s += fabsf(d) * bpt;
                    dout = G * (l2w * 2.0f * d * bpt + l1w * 10.0f * sgm * bpt * inv_nel);
                }
                s.dop[tid * 2 + c] = o > 0.0f ? dout : 0.0f;
            }
        }
        __syncthreads();
        // ---- hid_obs backwards
        for (int it = tid; it < Q * 24; it += NT) {
            const int row = it / 24, j = it % 24;
            s.du[row * 25 + j] = s.uu[row * 25 + j] > 0.0f ? w[W.H2 + j] * s.dop[row * 2] + w[W.H2 + 24 + j] * s.dop[row * 2 + 1] : 0.0f;
        }
        __syncthreads();
        float* dvv = s.D;                                            // [41][HS]: d loss / d (hid_obs' input rows)
        for (int it = tid; it < Q * H; it += NT) {
            const int row = it / H, k = it % H;
            float acc = 0.0f;
#pragma unroll 4
            for (int j = 0; j < 24; ++j) acc = fmaf(w[W.H0 + j * H + k], s.du[row * 25 + j], acc);
            dvv[row * HS + k] = acc;
        }
#pragma unroll
        for (int jj = 0; jj < NH0; ++jj) {                           // d hid_obs.0 [24][H + 1] += du (x) [v | 1] over the 41 rows
            const int i = tid + NT * jj;
            if (i < 24 * HS) {
                const int j = i / HS, k = i % HS;
                float acc = accH0[jj];
#pragma unroll 4
                for (int row = 0; row < Q; ++row) acc = fmaf(s.du[row * 25 + j], s.I[row * IS + k], acc);
                accH0[jj] = acc;
            }
        }
        if (tid < 50) {                                              // d hid_obs.2 [2][25] += dop (x) [relu(u) | 1]
            const int c = tid / 25, j = tid % 25;
#pragma unroll 4
            for (int row = 0; row < Q; ++row) accH2 = fmaf(s.dop[row * 2 + c], j < 24 ? s.uu[row * 25 + j] : 1.0f, accH2);
        }
        __syncthreads();
        // ---- gradient at the resampled particles and their log weights
        float dp1r = 0.0f;
        {
            float dot = 0.0f;
#pragma unroll 4
            for (int k = 0; k < H; ++k) dot = fmaf(dvv[P * HS + k], s.I[q * IS + k], dot);
            dp1r = dp + s.pi[q] * dot;
            if (tid < P) s.vtmp[tid] = dp1r;
        }
        for (int i = tid; i < P * H; i += NT) {
            const int p = i / H, k = i % H;
            s.dhr[p * RS + k] = s.dh[p * HS + k] + dvv[p * HS + k] + s.pi[p] * dvv[P * HS + k];
        }
        __syncthreads();
        {
            const float Ssum = st_sum40(s.vtmp);
            const float dpn = dp1r - s.pi[q] * Ssum;                 // through p1r = pn - logsumexp(pn)
            const float wj = rs_exp(s.vp1[s.vidx[q]]);
            if (tid < P) s.dhr[tid * RS + H] = st_div(dpn * floor_, al * wj + floor_);      // through pn = log(w / (alpha w + floor))
        }
        __syncthreads();
        // ---- back through the gather: every source particle sums its takers' rows in index order
        for (int it = tid; it < P * (H + 1); it += NT) {
            const int j = it / (H + 1), k = it % (H + 1);
            float acc = 0.0f;
#pragma unroll 4
            for (int i = 0; i < P; ++i)
                if (s.vidx[i] == j) acc += s.dhr[i * RS + k];
            if (k < H) s.dh1[j * HS + k] = acc;
            else s.vdp1[j] = acc;
        }
        __syncthreads();
        {
            const float dlp = s.vdp1[q] - rs_exp(s.vp1[q]) * st_sum40(s.vdp1);      // through p1 = lp - logsumexp(lp); also d / d p0
            dp = dlp;
            if (tid < P) s.vdlp[tid] = dlp;
        }
        __syncthreads();
        // ---- h1 = (1 - z) n + z h0, n = tanh(mu + eps softplus(var)); staging of d [mu | var] and [r h0 | x | 1]
        for (int i = tid; i < P * H; i += NT) {
            const int p = i / H, u = i % H;
            const float z = gz[i], r = gz[PH + i], n = gz[2 * PH + i], es = gz[3 * PH + i], h0 = hprev[i];
            const float h1 = (1.0f - z) * n + z * h0;
            const float d1 = fmaf(s.vdlp[p], w[W.O + u], s.dh1[p * HS + u]);
            const float dn = d1 * (1.0f - z);
            const float dm = dn * (1.0f - n * n);
            s.dh1[p * HS + u] = d1 * (h0 - n);                       // d z
            s.dh[p * HS + u] = d1 * z;                               // d h0, direct path
            s.dhr[p * RS + u] = h1;
            s.D[p * DS + u] = dm;
            s.D[p * DS + H + u] = dm * es;
            s.I[p * IS + u] = r * h0;
        }
        if (tid < P) {
#pragma unroll
            for (int k = 0; k < IN; ++k) s.I[tid * IS + H + k] = x[k];
            s.I[tid * IS + H + IN] = 1.0f;
        }
        __syncthreads();
        if (tid < C) {                                               // d fc_obs [H + 4] += dlp (x) [h1 | x | 1]
#pragma unroll 4
            for (int p = 0; p < P; ++p) accO = fmaf(s.vdlp[p], tid < H ? s.dhr[p * RS + tid] : s.I[p * IS + tid], accO);
        }
        outer_acc<RI, CJ>(s.D, DS, s.I, IS, ty, tx, accN);
        for (int it = tid; it < NPG * H; it += NT) {                 // d (r h0) = W_n[:, :H]^T d [mu | var]
            const int k = it % H, pg = it / H;
            float acc[PG];
            bw_product<H>(w + W.N, s.D, DS, k, pg, acc);
#pragma unroll
            for (int j = 0; j < PG; ++j) s.t1[(pg * PG + j) * HS + k] = acc[j];
        }
        __syncthreads();
        // ---- z, r = sigmoid(W_zr [h0, x] + b); staging of d (a_z | a_r) and [h0 | x | 1]
        for (int i = tid; i < P * H; i += NT) {
            const int p = i / H, u = i % H;
            const float z = gz[i], r = gz[PH + i], h0 = hprev[i];
            const float drh = s.t1[p * HS + u];
            s.dh[p * HS + u] = fmaf(drh, r, s.dh[p * HS + u]);
            const float dr = drh * h0;
            s.D[p * DS + u] = s.dh1[p * HS + u] * z * (1.0f - z);
            s.D[p * DS + H + u] = dr * r * (1.0f - r);
            s.I[p * IS + u] = h0;                                    // columns H .. H + 3 still hold x | 1
        }
        __syncthreads();
        outer_acc<RI, CJ>(s.D, DS, s.I, IS, ty, tx, accZR);
        for (int it = tid; it < NPG * H; it += NT) {                 // d h0 += W_zr[:, :H]^T d (a_z | a_r): the gradient at step t - 1's set
            const int k = it % H, pg = it / H;
            float acc[PG];
            bw_product<H>(w + W.ZR, s.D, DS, k, pg, acc);
#pragma unroll
            for (int j = 0; j < PG; ++j) s.dh[(pg * PG + j) * HS + k] += acc[j];
        }
        __syncthreads();
    }

    // ------------------------------------------------------------------------------------------ the episode's slab
#pragma unroll
    for (int i = 0; i < RI; ++i)
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            const int row = ty + 16 * i, col = tx + 16 * j;
            if (col < C) {
                g[G_.ZR + row * C + col] = accZR[i][j];
                g[G_.N + row * C + col] = accN[i][j];
            }
        }
#pragma unroll
    for (int jj = 0; jj < NH0; ++jj) {
        const int i = tid + NT * jj;
        if (i < 24 * HS) g[G_.H0 + i] = accH0[jj];
    }
    if (tid < 50) g[G_.H2 + tid] = accH2;
    if (tid < C) g[G_.O + tid] = accO;
    if (tid < G_.stride - G_.end) g[G_.end + tid] = 0.0f;            // the slab's padding
    if (tid == P) {
        const float pred = l2w * l2s + l1w * 10.0f * l1s * inv_nel;
        const float part = (l2w * l2ps + l1w * 10.0f * l1ps) * inv_nel;
        a_.loss[e] = G * (pred + elbo * part);
    }
}

template <int H>
void launch_pass(const StArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(rs_pfgru_sized_train_fwd_kernel<H>, dim3((unsigned)a.E), dim3(NT), 0, st, a);
    hipLaunchKernelGGL(rs_pfgru_sized_train_bwd_kernel<H>, dim3((unsigned)a.E), dim3(NT), 0, st, a);
}

}  // namespace

extern "C" {

int32_t rs_pfgru_sized_train_weight_floats(int32_t hidden) { return width_ok(hidden) ? (int32_t)wlayout(hidden).stride : 0; }
int32_t rs_pfgru_sized_train_grad_floats(int32_t hidden) { return width_ok(hidden) ? (int32_t)glayout(hidden).stride : 0; }

int rs_pfgru_sized_train(const float* weights, const float* obs, const float* target, const float* bp, const int64_t* lens, const float* w_ep,
                         const float* h0, const float* eps, const double* u, float* hs, float* ps, float* gates, int32_t* idx, float* loss,
                         float* grads, int32_t steps, int32_t episodes, double alpha, double l2_weight, double l1_weight, double elbo_weight,
                         int32_t hidden, rs_stream_t stream) {
    if (!width_ok(hidden) || !weights || !obs || !target || !bp || !lens || !w_ep || !h0 || !eps || !hs || !ps || !gates || !idx || !loss ||
        !grads || steps < 1 || episodes < 0)
        return RS_ERR_INVALID_ARG;
    if (episodes == 0) return RS_OK;
    const StArgs a{weights, obs, target, bp, lens, w_ep, h0, eps, u, hs, ps, gates, idx, loss, grads, steps, episodes, (float)alpha,
                   (float)((1.0 - alpha) / (double)P), (float)l2_weight, (float)l1_weight, (float)elbo_weight};
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (hidden) {
        case 8: launch_pass<8>(a, st); break;
        case 16: launch_pass<16>(a, st); break;
        case 24: launch_pass<24>(a, st); break;
        case 32: launch_pass<32>(a, st); break;
        case 40: launch_pass<40>(a, st); break;
        case 48: launch_pass<48>(a, st); break;
        case 56: launch_pass<56>(a, st); break;
        case 64: launch_pass<64>(a, st); break;
        default: return RS_ERR_INVALID_ARG;
    }
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

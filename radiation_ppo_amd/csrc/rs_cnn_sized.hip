// rs_cnn_sized.hip -- the RAD-TEAM CNN trunk of K9/K10 (rs_cnn.hip) for square heat maps of any side 8 <= M <= 256:
//     conv3x3(Cin->8, pad 1) - ReLU - maxpool 2x2/2 (floor: P = M / 2) - conv3x3(8->16, pad 1) - ReLU - flatten(16 P P)
// forward and weight-gradient backward, straight from the resident shared maps.  Without enforced walls the maps grow by about one
// cell a side per episode step (147 x 147 for 120-step episodes, maps.heat_map_geometry): one image's four input planes (346 KB at 147)
// no longer fit a CU's LDS, so the image is TILED:
//   * a workgroup (256 threads) owns a tile of 16 x 16 pooled cells = the 16 x 16 conv2 output pixels over them; a persistent grid
//     strides over the (image, tile) pairs;
//   * forward: conv2 over the tile needs P1 with a one-cell halo (18 x 18 pooled cells), that needs an input window of 2 * 16 + 6 = 38
//     pixels a side (4 planes, 23 KB of LDS); P1 cells outside [0, P) are conv2's zero padding and are not computed.  conv1 is evaluated
//     per pooled cell (a 4 x 4 window per plane feeds the cell's 2 x 2 conv pixels, 8 channels each), ReLU and max-pool in registers,
//     as in K9; conv2 has one thread per output pixel;
//   * the input stack is never materialised: as in K9/K10 the actor's two one-hot channels (prediction, location) enter conv1 as 3 x 3
//     weight stamps and dW1 as gathers, `others` = combined - location is convolved as `combined`;
//   * weights are read in torch's own layout through the scalar unit (wave-uniform addresses; 3.5 KB per network), so neither a
//     prepare step nor a weight scratch is needed;
//   * backward: dW2 = dZ2 x patches(P1) and db2 on threads (output channel, input channel, half tile), dP1 = conv2^T(dZ2) per pooled cell, gated by
//     P1 > 0, dW1 through the pool's arg-max (one of the four conv1 pixels of a cell carries gradient) on threads (output channel,
//     plane pair, tile row).  Accumulators stay in registers across all tiles of a workgroup, which writes one slab row at the end
//     (fixed-order reduction, no atomics: bit-identical from one run to the next);
//   * the Monte-Carlo evaluation's team forward (rs_sized_team_fwd, rs_cnn_sized_team_infer): every agent's actor trunk in one launch
//     over (image, tile, agent) units, the same unit function, conv1 skipped over empty input windows (bit for bit: fwd_unit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"

namespace {

constexpr int TS = 16;                       // pooled cells per tile side
constexpr int NT = TS * TS;                  // 256 threads: thread = pooled cell / conv2 output pixel of the tile
constexpr int HS = TS + 2;                   // 18: the tile's P1 / dZ2 with a one-cell halo
constexpr int HC = HS * HS;                  // 324 halo cells
constexpr int FWS = 2 * TS + 6;              // 38: forward input window side (conv1 over the halo cells), origin input (2 ty0 - 3, 2 tx0 - 3)
constexpr int BWS = 2 * TS + 2;              // 34: backward input window side (dW1 over the tile's own cells), origin (2 ty0 - 1, 2 tx0 - 1)
constexpr int C1 = 8, C2 = 16, DP = 4;       // conv1 / conv2 output channels; dense input planes (combined, readings, visits, obstacles)
constexpr int MIN_SIDE = 8, MAX_SIDE = 256;

typedef const float __attribute__((address_space(4))) * cmem_t;
__device__ __forceinline__ cmem_t as_cmem(const float* p) { return (cmem_t)(uintptr_t)p; }

struct SzIn {
    const float* maps;        // [S][4][M*M]
    const int64_t* cells;     // [S][A] owner cells (actor) or nullptr (critic)
    const int64_t* pcells;    // [S][A] prediction cell or -1
    int A, agent, M, P, ntile;
    long long S;
};

// the four dense planes of image s over the window [r0, r0 + W) x [c0, c0 + W) into LDS (zero outside the map), BATCH loads in flight
// per thread at a time (all ~20 at once held their 64-bit addresses too and pushed the forward kernel past its VGPR budget)
// Returns whether any staged element compares unequal to 0.0f (a NaN does, -0.0f does not): the team kernel's empty-window test; the
// other kernels drop the value and the compiler the comparisons.
template <int W>
__device__ __forceinline__ bool stage_window(const SzIn& in, long long s, int r0, int c0, float* xs) {
    constexpr int N = DP * W * W, PER = (N + NT - 1) / NT, BATCH = 8;
    const float* src = in.maps + (size_t)s * DP * in.M * in.M;
    bool nz = false;
#pragma unroll
    for (int i0 = 0; i0 < PER; i0 += BATCH) {
        float v[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            const int e = threadIdx.x + (i0 + i) * NT;
            const int d = e / (W * W), rem = e - d * (W * W), wr = rem / W, wc = rem - wr * W;
            const int r = r0 + wr, c = c0 + wc;
            v[i] = (i0 + i < PER && e < N && r >= 0 && r < in.M && c >= 0 && c < in.M) ? src[((size_t)d * in.M + r) * in.M + c] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            const int e = threadIdx.x + (i0 + i) * NT;
            if (i0 + i < PER && e < N) xs[e] = v[i];
            nz |= v[i] != 0.0f;
        }
    }
    return nz;
}

__device__ __forceinline__ void owner_cells(const SzIn& in, long long s, int& loc, int& pc) {
    loc = -1; pc = -1;
    if (in.agent >= 0) {
        loc = (int)in.cells[(size_t)s * in.A + in.agent];
        pc = (int)in.pcells[(size_t)s * in.A + in.agent];
    }
}

// ------------------------------------------------------------------------------------------------
// Forward: maps -> a2 [S][16 P P] (torch Flatten order c P P + y P + x); TRAIN also writes p1 [S][P P][8], amax [S][P P][8] (0..3,
// row-major, first maximum) and relu_mask [S][P P] (bit c = a2 channel c > 0), the schema of K9 with P P in place of 169.

// The LDS of a forward workgroup; stl [which][tap][co] holds the actor's one-hot stamps: prediction, location - others.
struct FwdLds {
    __align__(16) float xs[DP * FWS * FWS];                   // input window, [plane][38][38]
    float ps[C1 * HC];                                        // P1 with halo, [ci][18][18]
    float stl[2 * 9 * C1];
};

__device__ __forceinline__ void fwd_stamps(const float* __restrict__ w1, float* stl) {
    const int tid = threadIdx.x;
    if (tid < 2 * 9 * C1) {
        const int which = tid / (9 * C1), kk = (tid % (9 * C1)) / C1, co = tid % C1;
        stl[tid] = which == 0 ? w1[(co * 6 + 0) * 9 + kk] : w1[(co * 6 + 1) * 9 + kk] - w1[(co * 6 + 2) * 9 + kk];
    }
}

// One (image, tile) unit of the forward pass, by the whole workgroup; loc / pc: the owner's cells (-1: none), stl: its stamps.
// SKIP (the evaluation's team kernel): a unit whose staged window holds nothing but zeros and neither cell does not evaluate conv1.
// There every conv1 accumulator is +0 (they start at +0 and fmaf(w, +-0, +0) = +0), so every pooled cell inside the map is
// max(0 + b1, 0), the maximum of four equal values: the same bits.  One block-wide OR decides, uniform over the workgroup.
template <int CIN, bool TRAIN, bool SKIP>
__device__ __forceinline__ void fwd_unit(const SzIn& in, long long s, int tile, int loc, int pc, const float* __restrict__ w1,
                                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                         float* __restrict__ a2, float* __restrict__ p1g, uint8_t* __restrict__ amax,
                                         uint16_t* __restrict__ relu_mask, FwdLds& lds) {
    float* xs = lds.xs;
    float* ps = lds.ps;
    const float* stl = lds.stl;
    constexpr int CH0 = (CIN == 6) ? 2 : 0;                   // logical channel of dense plane 0 (actor: `others`, convolved as `combined`)
    const int tid = threadIdx.x, M = in.M, P = in.P, PP = P * P;
    const int ty0 = (tile / in.ntile) * TS, tx0 = (tile % in.ntile) * TS;
    // the weight addresses as values of this iteration: loop-invariant, hipcc hoisted the scalar weight loads out of the tile loop
    cmem_t w1c = as_cmem(w1), b1c = as_cmem(b1), w2c = as_cmem(w2), b2c = as_cmem(b2);
    asm volatile("" : "+s"(w1c), "+s"(b1c), "+s"(w2c), "+s"(b2c));
    const bool nz = stage_window<FWS>(in, s, 2 * ty0 - 3, 2 * tx0 - 3, xs);
    bool dense = true;
    if (SKIP) {
        auto inside = [&](int at) {
            const int r = at / M - (2 * ty0 - 3), c = at % M - (2 * tx0 - 3);
            return at >= 0 && r >= 0 && r < FWS && c >= 0 && c < FWS;
        };
        dense = __syncthreads_or(nz || inside(loc) || inside(pc)) != 0;
    } else {
        __syncthreads();
    }
    if (!dense) {
        for (int h = tid; h < HC; h += NT) {
            const int hy = h / HS, hx = h - hy * HS, gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            const bool in_map = gy >= 0 && gy < P && gx >= 0 && gx < P;
#pragma unroll
            for (int co = 0; co < C1; ++co) ps[co * HC + h] = in_map ? fmaxf(0.0f + b1c[co], 0.0f) : 0.0f;
        }
    }
    // ---- conv1 + bias + ReLU + max-pool for the 18 x 18 halo cells (two passes of the 256 threads)
#pragma unroll 1
    for (int h = tid; dense && h < HC; h += NT) {
        const int hy = h / HS, hx = h - hy * HS, gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
        if (gy < 0 || gy >= P || gx < 0 || gx >= P) {
#pragma unroll
            for (int co = 0; co < C1; ++co) ps[co * HC + h] = 0.0f;      // conv2's zero padding
            continue;
        }
        float acc[4][C1];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int co = 0; co < C1; ++co) acc[p][co] = 0.0f;
        // rolled over (plane, ky): each trip needs 24 weights (3 kx x 8 co) in SGPRs; unrolled, hipcc issued all 288 scalar loads
        // up front and spilled them
        const float* xw = xs + 2 * hy * FWS + 2 * hx;
#pragma unroll 1
        for (int q = 0; q < DP * 3; ++q) {
            const int d = q / 3, ky = q - d * 3;
            float win[2][4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float2 a = *reinterpret_cast<const float2*>(&xw[d * FWS * FWS + (i + ky) * FWS]);
                const float2 c = *reinterpret_cast<const float2*>(&xw[d * FWS * FWS + (i + ky) * FWS + 2]);
                win[i][0] = a.x; win[i][1] = a.y; win[i][2] = c.x; win[i][3] = c.y;
            }
            const cmem_t wq = w1c + (CH0 + d) * 9 + ky * 3;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int co = 0; co < C1; ++co) {
                    const float w = wq[co * CIN * 9 + kx];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i * 2 + j][co] = __builtin_fmaf(w, win[i][j + kx], acc[i * 2 + j][co]);
                }
        }
        if (CIN == 6) {
            // a 1 at input (r, c) adds w[ky][kx] to conv pixel (r - ky + 1, c - kx + 1)
            auto stamp = [&](int at, const float* ws) {
                const int r = at / M, c = at - r * M, dy = r - 2 * gy, dx = c - 2 * gx;
                if (dy >= -1 && dy <= 2 && dx >= -1 && dx <= 2) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int ky = dy - i + 1, kx = dx - j + 1;
                            if (ky >= 0 && ky < 3 && kx >= 0 && kx < 3)
#pragma unroll
                                for (int co = 0; co < C1; ++co) acc[i * 2 + j][co] += ws[(ky * 3 + kx) * C1 + co];
                        }
                }
            };
            if (loc >= 0) stamp(loc, stl + 9 * C1);       // -1: no position recorded yet (fresh maps), an empty one-hot
            if (pc >= 0) stamp(pc, stl);
        }
        const bool own = hy >= 1 && hy <= TS && hx >= 1 && hx <= TS;
        float best[C1];
        uint32_t pidx[2] = {0u, 0u};
#pragma unroll
        for (int co = 0; co < C1; ++co) {
            const float bb = b1c[co];
            float bv = fmaxf(acc[0][co] + bb, 0.0f);
            int idx = 0;
#pragma unroll
            for (int p = 1; p < 4; ++p) {
                const float v = fmaxf(acc[p][co] + bb, 0.0f);
                if (v > bv) { bv = v; idx = p; }
            }
            ps[co * HC + h] = bv;
            best[co] = bv;
            pidx[co >> 2] |= (uint32_t)idx << (8 * (co & 3));
        }
        if (TRAIN && own) {
            const size_t cell = (size_t)s * PP + gy * P + gx;
            float4* dst = reinterpret_cast<float4*>(p1g + cell * C1);
            dst[0] = make_float4(best[0], best[1], best[2], best[3]);
            dst[1] = make_float4(best[4], best[5], best[6], best[7]);
            *reinterpret_cast<uint2*>(amax + cell * C1) = make_uint2(pidx[0], pidx[1]);
        }
    }
    __syncthreads();
    // ---- conv2 + bias + ReLU: thread = output pixel
    {
        const int ly = tid / TS, lx = tid - ly * TS, oy = ty0 + ly, ox = tx0 + lx;
        if (oy < P && ox < P) {
            float acc2[C2];
#pragma unroll
            for (int co = 0; co < C2; ++co) acc2[co] = b2c[co];
            const float* pq = ps + ly * HS + lx;
#pragma unroll 1
            for (int q = 0; q < C1 * 3; ++q) {           // rolled over (ci, ky): 48 weights per trip
                const int ci = q / 3, ky = q - ci * 3;
                const cmem_t wq = w2c + ci * 9 + ky * 3;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = pq[ci * HC + ky * HS + kx];
#pragma unroll
                    for (int co = 0; co < C2; ++co) acc2[co] = __builtin_fmaf(wq[co * 72 + kx], v, acc2[co]);
                }
            }
            uint32_t live = 0u;
            float* dst = a2 + (size_t)s * C2 * PP + oy * P + ox;
#pragma unroll
            for (int co = 0; co < C2; ++co) {
                const float o = fmaxf(acc2[co], 0.0f);
                dst[(size_t)co * PP] = o;
                live |= (o > 0.0f ? 1u : 0u) << co;
            }
            if (TRAIN) relu_mask[(size_t)s * PP + oy * P + ox] = (uint16_t)live;
        }
    }
    // the next unit's staging writes xs (and the team kernel stl) only; ps is rewritten after the barrier behind that staging
}

template <int CIN, bool TRAIN>
__global__ void __launch_bounds__(NT, 3) rs_sized_trunk_fwd(SzIn in, const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ a2, float* __restrict__ p1g, uint8_t* __restrict__ amax,
                                                           uint16_t* __restrict__ relu_mask) {
    __shared__ FwdLds lds;
    if (CIN == 6) fwd_stamps(w1, lds.stl);
    const int nt2 = in.ntile * in.ntile;
    const long long units = in.S * nt2;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long s = u / nt2;
        int loc, pc;
        owner_cells(in, s, loc, pc);
        fwd_unit<CIN, TRAIN, false>(in, s, (int)(u - s * nt2), loc, pc, w1, b1, w2, b2, a2, p1g, amax, relu_mask, lds);
    }
}

// ------------------------------------------------------------------------------------------------
// The evaluation's team forward: every agent's actor trunk in one launch.  A persistent grid strides over the (image, tile, agent)
// units, the agent fastest: the workgroups that are resident together stage the same windows, which then come from L2.  The unit is
// fwd_unit's, so the bits are rs_sized_trunk_fwd<6, false>'s with the agent's weights; the cells come from the heat maps' own int32
// fields.  168 VGPRs (three workgroups per CU, as the forward kernel), 34 KB of LDS.
struct SzTeam {
    rs_cnn_conv_params conv[RS_MAX_AGENTS];   // in the kernel's argument block (8 agents x 4 pointers = 256 bytes)
    const int32_t* cells;                     // [S][A]
    const int32_t* pcells;                    // [S][A]
};

__global__ void __launch_bounds__(NT, 3) rs_sized_team_fwd(SzIn in, SzTeam team, float* __restrict__ a2) {
    __shared__ FwdLds lds;
    const int nt2 = in.ntile * in.ntile, A = in.A;
    const long long units = in.S * nt2 * A;
    const size_t per_agent = (size_t)in.S * C2 * in.P * in.P;
    int stamped = -1;                          // the agent whose stamps stl holds
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long it = u / A, s = it / nt2;
        const int a = (int)(u - it * A);
        const rs_cnn_conv_params cv = team.conv[a];
        const int loc = team.cells[(size_t)s * A + a], pc = team.pcells[(size_t)s * A + a];
        if (a != stamped) fwd_stamps(cv.w1, lds.stl);      // the last unit's conv1 has read its stamps: a barrier lies behind every conv1
        stamped = a;
        fwd_unit<6, false, true>(in, s, (int)(it - s * nt2), loc, pc, cv.w1, cv.b1, cv.w2, cv.b2, a2 + (size_t)a * per_agent, nullptr, nullptr,
                                 nullptr, lds);
    }
}

// The training round's critic team forward (rs_cnn_sized_team_critic_infer): every critic's trunk in one launch, the Cin = 4 form of the
// kernel above -- no cell planes, no stamps -- over (image, tile, critic) units, the critic fastest.  The unit is fwd_unit's with the
// empty-window shortcut, so the bits are rs_sized_trunk_fwd<4, false>'s with the critic's weights.
struct SzCritics {
    rs_cnn_conv_params conv[RS_MAX_AGENTS];
};

__global__ void __launch_bounds__(NT, 3) rs_sized_critics_fwd(SzIn in, SzCritics team, float* __restrict__ a2) {
    __shared__ FwdLds lds;
    const int nt2 = in.ntile * in.ntile, C = in.A;                   // in.A: the number of critics
    const long long units = in.S * nt2 * C;
    const size_t per_critic = (size_t)in.S * C2 * in.P * in.P;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long it = u / C, s = it / nt2;
        const int c = (int)(u - it * C);
        const rs_cnn_conv_params cv = team.conv[c];
        fwd_unit<4, false, true>(in, s, (int)(it - s * nt2), -1, -1, cv.w1, cv.b1, cv.w2, cv.b2, a2 + (size_t)c * per_critic, nullptr, nullptr,
                                 nullptr, lds);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward: dL/d(a2) -> per-workgroup partial sums, slab row {dW1 8*CIN*9 | db1 8 | dW2 16*72 | db2 16} in torch weight order.
template <int CIN>
__global__ void __launch_bounds__(NT, 2) rs_sized_trunk_bwd(SzIn in, const float* __restrict__ w2, const float* __restrict__ da2,
                                                           const uint16_t* __restrict__ relu_mask, const float* __restrict__ p1g,
                                                           const uint8_t* __restrict__ amax, float* __restrict__ slab) {
    __shared__ __align__(16) float smem[DP * BWS * BWS + C1 * HC + C2 * HC + C1 * NT + 2 * NT];
    float* xs = smem;                         // input window [plane][34][34]
    float* ps = xs + DP * BWS * BWS;          // P1 with halo [ci][18][18]
    float* dz = ps + C1 * HC;                 // dZ2 = ReLU-gated da2 with halo [co][18][18]
    float* gb = dz + C2 * HC;                 // dL/d(P1) gated by P1 > 0, the tile's cells [ci][256]
    uint8_t* am = reinterpret_cast<uint8_t*>(gb + C1 * NT);     // arg-max codes of the tile's cells [256][8]
    constexpr int K1 = CIN * 9, CH0 = (CIN == 6) ? 2 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = in.P, PP = P * P;
    const int ly = tid / TS, lx = tid - ly * TS;
    // dW2 / db2: thread = (output channel co2, input channel ci2, half of the tile's rows) -> 9 taps + db2;
    // dW1 / db1: thread = (output channel co1, plane pair, tile row ly) -> 2 x 9 taps + db1
    const int co2 = tid & 15, ci2 = (tid >> 4) & 7, half2 = tid >> 7;
    const int co1 = tid & 7, half = (tid >> 3) & 1;
    float aw2[10], aw1[19], gst = 0.0f;
#pragma unroll
    for (int k = 0; k < 10; ++k) aw2[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 19; ++k) aw1[k] = 0.0f;
    const int nt2 = in.ntile * in.ntile;
    const long long units = in.S * nt2;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long s = u / nt2;
        const int tile = (int)(u - s * nt2), ty0 = (tile / in.ntile) * TS, tx0 = (tile % in.ntile) * TS;
        int loc, pc;
        owner_cells(in, s, loc, pc);
        cmem_t w2c = as_cmem(w2);                 // per iteration, as in the forward kernel
        asm volatile("" : "+s"(w2c));
        stage_window<BWS>(in, s, 2 * ty0 - 1, 2 * tx0 - 1, xs);
#pragma unroll 1
        for (int h = tid; h < HC; h += NT) {
            const int hy = h / HS, hx = h - hy * HS, gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            const bool in_map = gy >= 0 && gy < P && gx >= 0 && gx < P;
            const size_t cell = (size_t)s * PP + (in_map ? gy * P + gx : 0);
            float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pb = pa;
            uint32_t live = 0u;
            if (in_map) {
                pa = reinterpret_cast<const float4*>(p1g + cell * C1)[0];
                pb = reinterpret_cast<const float4*>(p1g + cell * C1)[1];
                live = relu_mask[cell];
            }
            ps[0 * HC + h] = pa.x; ps[1 * HC + h] = pa.y; ps[2 * HC + h] = pa.z; ps[3 * HC + h] = pa.w;
            ps[4 * HC + h] = pb.x; ps[5 * HC + h] = pb.y; ps[6 * HC + h] = pb.z; ps[7 * HC + h] = pb.w;
            const float* g = da2 + (size_t)s * C2 * PP + (in_map ? gy * P + gx : 0);
#pragma unroll
            for (int co = 0; co < C2; ++co) dz[co * HC + h] = ((live >> co) & 1u) ? g[(size_t)co * PP] : 0.0f;
        }
        {
            const int gy = ty0 + ly, gx = tx0 + lx;
            uint2 code = make_uint2(0u, 0u);
            if (gy < P && gx < P) code = *reinterpret_cast<const uint2*>(amax + ((size_t)s * PP + gy * P + gx) * C1);
            *reinterpret_cast<uint2*>(am + tid * C1) = code;
        }
        __syncthreads();
        // ---- dW2[co][ci][ky][kx] += sum_px dZ2[co][px] P1[ci][px + (ky - 1, kx - 1)], db2[co] += sum_px dZ2[co][px]: eight rows of 16
        // pixels; a P1 row of 18 values serves the three kx taps of all 16 pixels of a row
#pragma unroll 1
        for (int yy = 0; yy < TS / 2; ++yy) {
            const int y = half2 * (TS / 2) + yy;
            float dzr[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) { dzr[x] = dz[co2 * HC + (y + 1) * HS + x + 1]; aw2[9] += dzr[x]; }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                float r[HS];
#pragma unroll
                for (int x = 0; x < HS; ++x) r[x] = ps[ci2 * HC + (y + ky) * HS + x];
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int x = 0; x < TS; ++x) aw2[ky * 3 + kx] = __builtin_fmaf(dzr[x], r[x + kx], aw2[ky * 3 + kx]);
            }
        }
        // ---- dP1[ci][cell] = sum_{co,ky,kx} w2[co][ci][ky][kx] dZ2[co][cell - (ky - 1, kx - 1)], gated by P1 > 0 (cells outside the map have
        // P1 = 0 in ps: no gradient)
        {
            float g[C1];
#pragma unroll
            for (int ci = 0; ci < C1; ++ci) g[ci] = 0.0f;
            const float* dq = dz + (ly + 2) * HS + lx + 2;
#pragma unroll 1
            for (int q = 0; q < C2 * 3; ++q) {               // rolled over (co, ky): 24 weights per trip
                const int co = q / 3, ky = q - co * 3;
                const cmem_t wq = w2c + co * 72 + ky * 3;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = dq[co * HC - ky * HS - kx];
#pragma unroll
                    for (int ci = 0; ci < C1; ++ci) g[ci] = __builtin_fmaf(wq[ci * 9 + kx], v, g[ci]);
                }
            }
#pragma unroll
            for (int ci = 0; ci < C1; ++ci) gb[ci * NT + tid] = ps[ci * HC + (ly + 1) * HS + lx + 1] > 0.0f ? g[ci] : 0.0f;
        }
        __syncthreads();
        // ---- dW1[co1][plane][ky][kx] += g[co1][cell] x[plane] at the cell's arg-max pixel + (ky - 1, kx - 1); db1[co1] += g
        {
#pragma unroll 1
            for (int x = 0; x < TS; ++x) {
                const int cell = ly * TS + x;
                const float gv = gb[co1 * NT + cell];
                const int code = am[cell * C1 + co1];
                const float* base = xs + (2 * half) * BWS * BWS + (2 * ly + (code >> 1)) * BWS + 2 * x + (code & 1);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int kk = 0; kk < 9; ++kk) aw1[j * 9 + kk] = __builtin_fmaf(gv, base[j * BWS * BWS + (kk / 3) * BWS + kk % 3], aw1[j * 9 + kk]);
                aw1[18] += gv;
            }
        }
        if (CIN == 6 && tid < 2 * C1 * 9) {
            // the one-hot channels: input (r, c) meets tap (ky, kx) at conv pixel (r - ky + 1, c - kx + 1), which carries gradient iff it
            // is its pool window's arg-max for channel co; the tile that owns the pooled cell adds it
            const int which = tid / (C1 * 9), co = (tid % (C1 * 9)) / 9, kk = tid % 9;
            const int at = which ? loc : pc;
            if (at >= 0) {
                const int r = at / in.M, c = at - r * in.M;
                const int y = r - kk / 3 + 1, x = c - kk % 3 + 1;
                if (y >= 0 && y < 2 * P && x >= 0 && x < 2 * P) {
                    const int cy = (y >> 1) - ty0, cx = (x >> 1) - tx0;
                    if (cy >= 0 && cy < TS && cx >= 0 && cx < TS && am[(cy * TS + cx) * C1 + co] == (uint8_t)((y & 1) * 2 + (x & 1)))
                        gst += gb[co * NT + cy * TS + cx];
                }
            }
        }
        __syncthreads();
    }
    // ---- workgroup reduction in a fixed order.  dW1: the four tile rows of a wave by lane swaps (lanes l, l ^ 16, l ^ 32), then the
    // four waves; dW2: the two row halves
#pragma unroll
    for (int k = 0; k < 19; ++k) { aw1[k] += __shfl_xor(aw1[k], 16); aw1[k] += __shfl_xor(aw1[k], 32); }
    float* red2 = smem;                        // [2 halves][8 ci][16 co][10]
    float* red1 = red2 + NT * 10;              // [4 waves][16 (co1, half)][19]
    float* gred = red1 + 4 * 16 * 19;          // [2][8][9]
#pragma unroll
    for (int k = 0; k < 10; ++k) red2[tid * 10 + k] = aw2[k];
    if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 19; ++k) red1[(wave * 16 + lane) * 19 + k] = aw1[k];
    }
    if (tid < 2 * C1 * 9) gred[tid] = gst;
    __syncthreads();
    constexpr int ROW = C1 * K1 + C1 + C2 * 72 + C2;
    float* out = slab + (size_t)blockIdx.x * ROW;
    for (int e = tid; e < ROW; e += NT) {
        float sum = 0.0f;
        if (e < C1 * K1) {
            const int o1 = e / K1, k = e - o1 * K1, i0 = k / 9, kk = k - i0 * 9;     // i0: the logical input channel
            if (i0 < CH0) { out[e] = gred[(i0 * C1 + o1) * 9 + kk]; continue; }   // prediction (0) / location (1): the stamp gathers
            const int d = i0 - CH0, combo = o1 + 8 * (d >> 1), slot = (d & 1) * 9 + kk;
            if (CIN == 6 && d == 0) sum = -gred[(C1 + o1) * 9 + kk];                 // others = combined - location
#pragma unroll
            for (int w = 0; w < 4; ++w) sum += red1[(w * 16 + combo) * 19 + slot];
        } else if (e < C1 * K1 + C1) {
            const int o1 = e - C1 * K1;
#pragma unroll
            for (int w = 0; w < 4; ++w) sum += red1[(w * 16 + o1) * 19 + 18];
        } else if (e < C1 * K1 + C1 + C2 * 72) {
            const int q = e - (C1 * K1 + C1), co = q / 72, k = q - co * 72, ci = k / 9, kk = k - ci * 9;
            sum = red2[(ci * 16 + co) * 10 + kk] + red2[(NT / 2 + ci * 16 + co) * 10 + kk];
        } else {
            const int co = e - (C1 * K1 + C1 + C2 * 72);
            sum = red2[co * 10 + 9] + red2[(NT / 2 + co) * 10 + 9];
        }
        out[e] = sum;
    }
}

// persistent grid: as many workgroups as are resident at once (occupancy query x CU count), each strides over the (image, tile) pairs
template <typename K>
inline int sized_grid(K kernel, long long units) {
    int per_cu = 0, dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, NT, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    const long long cap = (long long)cus * per_cu;
    return (int)(units < cap ? units : cap);
}

inline bool side_ok(int32_t M) { return M >= MIN_SIDE && M <= MAX_SIDE; }
inline int tiles(int32_t M) { return (M / 2 + TS - 1) / TS; }

int sized_forward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent, int64_t num_samples,
                  int32_t M, const float* w1, const float* b1, const float* w2, const float* b2, float* a2, float* p1, uint8_t* amax,
                  uint16_t* relu_mask, rs_stream_t stream) {
    if (!maps || !w1 || !b1 || !w2 || !b2 || !a2 || num_samples < 0) return RS_ERR_INVALID_ARG;
    if ((p1 == nullptr) != (amax == nullptr) || (p1 == nullptr) != (relu_mask == nullptr)) return RS_ERR_INVALID_ARG;
    if (agent >= 0 && (!cells || !pcells || agent >= num_agents)) return RS_ERR_INVALID_ARG;
    if (!side_ok(M)) return RS_ERR_UNSUPPORTED;
    if (num_samples == 0) return RS_OK;
    SzIn in{maps, cells, pcells, num_agents, agent, M, M / 2, tiles(M), (long long)num_samples};
    const long long units = (long long)num_samples * in.ntile * in.ntile;
    hipStream_t s = (hipStream_t)stream;
    const bool train = p1 != nullptr;
#define SZ_FWD(CIN, TRAIN) hipLaunchKernelGGL((rs_sized_trunk_fwd<CIN, TRAIN>), dim3(sized_grid(rs_sized_trunk_fwd<CIN, TRAIN>, units)), dim3(NT), 0, s, \
                                              in, w1, b1, w2, b2, a2, p1, amax, relu_mask)
    if (agent >= 0) { if (train) SZ_FWD(6, true); else SZ_FWD(6, false); }
    else { if (train) SZ_FWD(4, true); else SZ_FWD(4, false); }
#undef SZ_FWD
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // namespace

extern "C" {

int32_t rs_cnn_sized_slab_row(int32_t in_channels) {
    if (in_channels != 6 && in_channels != 4) return 0;
    return C1 * in_channels * 9 + C1 + C2 * 72 + C2;
}

int32_t rs_cnn_sized_slab_rows(int64_t num_samples, int32_t map_side, int32_t in_channels) {
    if (!side_ok(map_side) || num_samples <= 0 || (in_channels != 6 && in_channels != 4)) return 0;
    const long long units = (long long)num_samples * tiles(map_side) * tiles(map_side);
    return in_channels == 6 ? sized_grid(rs_sized_trunk_bwd<6>, units) : sized_grid(rs_sized_trunk_bwd<4>, units);
}

int rs_cnn_sized_forward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                         int64_t num_samples, int32_t map_side, const float* w1, const float* b1, const float* w2, const float* b2,
                         float* a2, float* p1, uint8_t* amax, uint16_t* relu_mask, rs_stream_t stream) {
    return sized_forward(maps, cells, pcells, num_agents, agent, num_samples, map_side, w1, b1, w2, b2, a2, p1, amax, relu_mask, stream);
}

int rs_cnn_sized_infer(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent, int64_t num_samples,
                       int32_t map_side, const float* w1, const float* b1, const float* w2, const float* b2, float* a2, rs_stream_t stream) {
    return sized_forward(maps, cells, pcells, num_agents, agent, num_samples, map_side, w1, b1, w2, b2, a2, nullptr, nullptr, nullptr,
                         stream);
}

int rs_cnn_sized_team_infer(const float* maps, const int32_t* cells, const int32_t* pcells, int32_t num_agents, int64_t num_samples,
                            int32_t map_side, const rs_cnn_conv_params* convs, float* a2, rs_stream_t stream) {
    if (!maps || !cells || !pcells || !convs || !a2 || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_samples < 0) return RS_ERR_INVALID_ARG;
    for (int a = 0; a < num_agents; ++a)
        if (!convs[a].w1 || !convs[a].b1 || !convs[a].w2 || !convs[a].b2) return RS_ERR_INVALID_ARG;
    if (!side_ok(map_side)) return RS_ERR_UNSUPPORTED;
    if (num_samples == 0) return RS_OK;
    SzIn in{maps, nullptr, nullptr, num_agents, 0, map_side, map_side / 2, tiles(map_side), (long long)num_samples};
    SzTeam team;
    for (int a = 0; a < RS_MAX_AGENTS; ++a) team.conv[a] = convs[a < num_agents ? a : 0];     // the slots behind the team repeat agent 0 (never read)
    team.cells = cells;
    team.pcells = pcells;
    const long long units = (long long)num_samples * in.ntile * in.ntile * num_agents;
    hipLaunchKernelGGL(rs_sized_team_fwd, dim3(sized_grid(rs_sized_team_fwd, units)), dim3(NT), 0, (hipStream_t)stream, in, team, a2);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_sized_team_critic_infer(const float* maps, int32_t num_critics, int64_t num_samples, int32_t map_side,
                                   const rs_cnn_conv_params* convs, float* a2, rs_stream_t stream) {
    if (!maps || !convs || !a2 || num_critics < 1 || num_critics > RS_MAX_AGENTS || num_samples < 0) return RS_ERR_INVALID_ARG;
    for (int c = 0; c < num_critics; ++c)
        if (!convs[c].w1 || !convs[c].b1 || !convs[c].w2 || !convs[c].b2) return RS_ERR_INVALID_ARG;
    if (!side_ok(map_side)) return RS_ERR_UNSUPPORTED;
    if (num_samples == 0) return RS_OK;
    SzIn in{maps, nullptr, nullptr, num_critics, -1, map_side, map_side / 2, tiles(map_side), (long long)num_samples};
    SzCritics team;
    for (int c = 0; c < RS_MAX_AGENTS; ++c) team.conv[c] = convs[c < num_critics ? c : 0];    // the slots behind the critics repeat critic 0 (never read)
    const long long units = (long long)num_samples * in.ntile * in.ntile * num_critics;
    hipLaunchKernelGGL(rs_sized_critics_fwd, dim3(sized_grid(rs_sized_critics_fwd, units)), dim3(NT), 0, (hipStream_t)stream, in, team, a2);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_sized_backward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                          int64_t num_samples, int32_t map_side, const float* w2, const float* da2, const uint16_t* relu_mask,
                          const float* p1, const uint8_t* amax, float* slab, int32_t slab_rows, rs_stream_t stream) {
    if (!maps || !w2 || !da2 || !relu_mask || !p1 || !amax || !slab || num_samples <= 0) return RS_ERR_INVALID_ARG;
    if (agent >= 0 && (!cells || !pcells || agent >= num_agents)) return RS_ERR_INVALID_ARG;
    if (!side_ok(map_side)) return RS_ERR_UNSUPPORTED;
    const int cin = agent >= 0 ? 6 : 4;
    const int grid = rs_cnn_sized_slab_rows(num_samples, map_side, cin);
    if (slab_rows < grid) return RS_ERR_INVALID_ARG;            // the slab must hold one row per workgroup
    SzIn in{maps, cells, pcells, num_agents, agent, map_side, map_side / 2, tiles(map_side), (long long)num_samples};
    hipStream_t s = (hipStream_t)stream;
    if (agent >= 0) hipLaunchKernelGGL(rs_sized_trunk_bwd<6>, dim3(grid), dim3(NT), 0, s, in, w2, da2, relu_mask, p1, amax, slab);
    else hipLaunchKernelGGL(rs_sized_trunk_bwd<4>, dim3(grid), dim3(NT), 0, s, in, w2, da2, relu_mask, p1, amax, slab);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

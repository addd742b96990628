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
//     over (image, tile, agent) units, the same unit function, conv1 skipped over empty input windows (bit for bit: fwd_unit);
//   * the occupancy-aware training passes (rs_sized_occupancy once per update, rs_sized_trunk_fwd_occ, rs_sized_trunk_bwd_occ): walls-off
//     maps are mostly empty and do not change over an update's iterations, so the units whose window is all zero are flagged once; the
//     forward then writes such a unit's constants and the backward reduces it to a few sums of dZ2 (see the kernels).
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

// The occupancy-aware training passes: a unit is empty when its forward window (38 x 38 pixels of the four planes, clipped to the map)
// holds nothing but zeros -- bit 0 of its flag, written once per update by rs_sized_occupancy -- and neither of the owner's cells.  The
// rule of fwd_unit's SKIP branch; the backward's 34 x 34 window and the 18 x 18 P1 halo lie inside that window, so one flag serves both.
// The flag is tested first and alone: an occupied window then never waits for the owner's cells, which the dense unit needs late.
__device__ __forceinline__ bool unit_is_empty(const SzIn& in, uint8_t flag, int ty0, int tx0, int loc, int pc) {
    if (flag & 1) return false;
    auto inside = [&](int at) {
        const int r = at / in.M - (2 * ty0 - 3), c = at % in.M - (2 * tx0 - 3);
        return at >= 0 && r >= 0 && r < FWS && c >= 0 && c < FWS;
    };
    return !inside(loc) && !inside(pc);
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
// CALLER: a second kernel that calls the same instantiation changes hipcc's inlining order and with it the first kernel's schedule;
// rs_sized_trunk_fwd_occ therefore takes an instantiation of its own (1) and leaves rs_sized_trunk_fwd's code as it was.
template <int CIN, bool TRAIN, bool SKIP, int CALLER = 0>
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
    constexpr bool OCC = false;
    const uint8_t* flags = nullptr;
#include "rs_cnn_sized_bwd.inc"
}

// The occupancy-aware backward.  An empty unit's inputs are zero and its P1 is the per-channel constant c1 = max(0 + b1, 0) inside the
// map, so with dZ2 = da2 gated by relu_mask (zero outside the map) its contributions are
//   db2[co]             += sum of dZ2[co] over the tile's pixels                                  (= S[co][1][1])
//   dW2[co][ci][ky][kx] += c1[ci] S[co][ky][kx],   S = sum of dZ2[co][y][x] over the pixels whose neighbour (y + ky - 1, x + kx - 1) is in the map
//   db1[ci]             += [c1[ci] > 0] sum_{co,ky,kx} w2[co][ci][ky][kx] R[co][ky][kx],   R = sum over own cells of dZ2[co][cy - ky + 1][cx - kx + 1]
//   dW1                 += 0 (the one-hot gathers too: neither owner cell is in the window)
// S and R are summed in registers over a workgroup's empty units, c1 and w2 folded in once in front of the slab row.  The slab's layout
// and rows are the dense kernel's; the sums are reassociated, not bit-identical to it, and bit-identical from one call to the next.
template <int CIN>
__global__ void __launch_bounds__(NT, 2) rs_sized_trunk_bwd_occ(SzIn in, const float* __restrict__ w2, const float* __restrict__ da2,
                                                               const uint16_t* __restrict__ relu_mask, const float* __restrict__ p1g,
                                                               const uint8_t* __restrict__ amax, const uint8_t* __restrict__ flags,
                                                               float* __restrict__ slab) {
    constexpr bool OCC = true;
#include "rs_cnn_sized_bwd.inc"
}

// The occupancy-aware training forward: fwd_unit for the occupied units; an empty unit neither stages its window nor evaluates conv1
// (p1 = c1, amax = 0, the first of four equal values), and its conv2 outputs are one of 9 x 16 values: a pixel's 3 x 3 P1 neighbourhood is
// c1 where it lies inside the map and conv2's zero padding outside, so only the pixel's place (first / inner / last row x column of the
// map) matters.  Thread (pattern, co) evaluates dense conv2's fmaf chain -- b2, then (ci, ky, kx) in order -- once per launch and keeps
// the result in a register; an empty unit broadcasts the table through ps.  Bit-identical to rs_sized_trunk_fwd<CIN, true>.
template <int CIN>
__global__ void __launch_bounds__(NT, 3) rs_sized_trunk_fwd_occ(SzIn in, const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, const float* __restrict__ b2,
                                                               float* __restrict__ a2, float* __restrict__ p1g, uint8_t* __restrict__ amax,
                                                               uint16_t* __restrict__ relu_mask, const uint8_t* __restrict__ flags) {
    __shared__ FwdLds lds;
    if (CIN == 6) fwd_stamps(w1, lds.stl);
    const int tid = threadIdx.x, P = in.P, PP = P * P;
    float ev = 0.0f;
    if (tid < 9 * C2) {
        const int pat = tid / C2, co = tid - pat * C2, py = pat / 3, px = pat - py * 3;      // 0: first row / column, 1: inner, 2: last
        float acc = b2[co];
        for (int ci = 0; ci < C1; ++ci) {
            const float c = fmaxf(0.0f + b1[ci], 0.0f);
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const bool in_map = !(py == 0 && ky == 0) && !(py == 2 && ky == 2) && !(px == 0 && kx == 0) && !(px == 2 && kx == 2);
                    acc = __builtin_fmaf(w2[co * 72 + ci * 9 + ky * 3 + kx], in_map ? c : 0.0f, acc);
                }
        }
        ev = fmaxf(acc, 0.0f);
    }
    bool table = false;                        // ps holds the table (the last unit was empty too)
    const int nt2 = in.ntile * in.ntile;
    const long long units = in.S * nt2;
    uint8_t ahead = blockIdx.x < units ? flags[blockIdx.x] : 1;      // a unit's flag is read one unit ahead: no unit starts with a wait for it
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const uint8_t flag = ahead;
        if (u + gridDim.x < units) ahead = flags[u + gridDim.x];
        const long long s = u / nt2;
        const int tile = (int)(u - s * nt2), ty0 = (tile / in.ntile) * TS, tx0 = (tile % in.ntile) * TS;
        int loc, pc;
        owner_cells(in, s, loc, pc);
        if (!unit_is_empty(in, flag, ty0, tx0, loc, pc)) {
            fwd_unit<CIN, true, false, 1>(in, s, tile, loc, pc, w1, b1, w2, b2, a2, p1g, amax, relu_mask, lds);
            table = false;
            continue;
        }
        if (!table) {
            __syncthreads();                   // the last unit's conv2 has read ps
            if (tid < 9 * C2) lds.ps[tid] = ev;
            __syncthreads();
            table = true;
        }
        const int ly = tid / TS, lx = tid - ly * TS, oy = ty0 + ly, ox = tx0 + lx;
        if (oy < P && ox < P) {
            cmem_t b1c = as_cmem(b1);
            const size_t cell = (size_t)s * PP + oy * P + ox;
            float c[C1];
#pragma unroll
            for (int co = 0; co < C1; ++co) c[co] = fmaxf(0.0f + b1c[co], 0.0f);
            float4* dst1 = reinterpret_cast<float4*>(p1g + cell * C1);
            dst1[0] = make_float4(c[0], c[1], c[2], c[3]);
            dst1[1] = make_float4(c[4], c[5], c[6], c[7]);
            *reinterpret_cast<uint2*>(amax + cell * C1) = make_uint2(0u, 0u);
            const int pat = ((oy == 0 ? 0 : oy == P - 1 ? 2 : 1) * 3 + (ox == 0 ? 0 : ox == P - 1 ? 2 : 1)) * C2;
            uint32_t live = 0u;
            float* dst = a2 + (size_t)s * C2 * PP + oy * P + ox;
#pragma unroll
            for (int co = 0; co < C2; ++co) {
                const float o = lds.ps[pat + co];
                dst[(size_t)co * PP] = o;
                live |= (o > 0.0f ? 1u : 0u) << co;
            }
            relu_mask[cell] = (uint16_t)live;
        }
    }
}

// flags [S][tiles]: bit 0 = the unit's forward window, clipped to the map, holds an element != 0.0f (a NaN does, -0.0f does not).  One
// read of the maps (the windows overlap by 6 of 38 pixels a side; the second read of an overlap comes from the cache).
__global__ void __launch_bounds__(NT) rs_sized_occupancy(SzIn in, uint8_t* __restrict__ flags) {
    const int nt2 = in.ntile * in.ntile, M = in.M;
    const long long units = in.S * nt2;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long s = u / nt2;
        const int tile = (int)(u - s * nt2), r0 = 2 * (tile / in.ntile) * TS - 3, c0 = 2 * (tile % in.ntile) * TS - 3;
        const float* src = in.maps + (size_t)s * DP * M * M;
        bool nz = false;
        for (int e = threadIdx.x; e < DP * FWS * FWS; e += NT) {
            const int d = e / (FWS * FWS), rem = e - d * (FWS * FWS), wr = rem / FWS, r = r0 + wr, c = c0 + rem - wr * FWS;
            if (r >= 0 && r < M && c >= 0 && c < M) nz |= src[((size_t)d * M + r) * M + c] != 0.0f;
        }
        const int any = __syncthreads_or(nz);
        if (threadIdx.x == 0) flags[u] = any ? 1 : 0;
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

int32_t rs_cnn_sized_tiles(int32_t map_side) { return side_ok(map_side) ? tiles(map_side) * tiles(map_side) : 0; }

int rs_cnn_sized_occupancy(const float* maps, int64_t num_samples, int32_t map_side, uint8_t* flags, rs_stream_t stream) {
    if (!maps || !flags || num_samples < 0) return RS_ERR_INVALID_ARG;
    if (!side_ok(map_side)) return RS_ERR_UNSUPPORTED;
    if (num_samples == 0) return RS_OK;
    SzIn in{maps, nullptr, nullptr, 0, -1, map_side, map_side / 2, tiles(map_side), (long long)num_samples};
    const long long units = (long long)num_samples * in.ntile * in.ntile, cap = 1 << 20;
    hipLaunchKernelGGL(rs_sized_occupancy, dim3((unsigned)(units < cap ? units : cap)), dim3(NT), 0, (hipStream_t)stream, in, flags);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_sized_forward_occ(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                             int64_t num_samples, int32_t map_side, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* a2, float* p1, uint8_t* amax, uint16_t* relu_mask, const uint8_t* flags, rs_stream_t stream) {
    if (!maps || !w1 || !b1 || !w2 || !b2 || !a2 || !p1 || !amax || !relu_mask || !flags || num_samples < 0) return RS_ERR_INVALID_ARG;
    if (agent >= 0 && (!cells || !pcells || agent >= num_agents)) return RS_ERR_INVALID_ARG;
    if (!side_ok(map_side)) return RS_ERR_UNSUPPORTED;
    if (num_samples == 0) return RS_OK;
    SzIn in{maps, cells, pcells, num_agents, agent, map_side, map_side / 2, tiles(map_side), (long long)num_samples};
    const long long units = (long long)num_samples * in.ntile * in.ntile;
    hipStream_t s = (hipStream_t)stream;
    if (agent >= 0)
        hipLaunchKernelGGL(rs_sized_trunk_fwd_occ<6>, dim3(sized_grid(rs_sized_trunk_fwd_occ<6>, units)), dim3(NT), 0, s, in, w1, b1, w2, b2, a2,
                           p1, amax, relu_mask, flags);
    else
        hipLaunchKernelGGL(rs_sized_trunk_fwd_occ<4>, dim3(sized_grid(rs_sized_trunk_fwd_occ<4>, units)), dim3(NT), 0, s, in, w1, b1, w2, b2, a2,
                           p1, amax, relu_mask, flags);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_cnn_sized_backward_occ(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                              int64_t num_samples, int32_t map_side, const float* w2, const float* da2, const uint16_t* relu_mask,
                              const float* p1, const uint8_t* amax, float* slab, int32_t slab_rows, const uint8_t* flags,
                              rs_stream_t stream) {
    if (!maps || !w2 || !da2 || !relu_mask || !p1 || !amax || !slab || !flags || num_samples <= 0) return RS_ERR_INVALID_ARG;
    if (agent >= 0 && (!cells || !pcells || agent >= num_agents)) return RS_ERR_INVALID_ARG;
    if (!side_ok(map_side)) return RS_ERR_UNSUPPORTED;
    // the dense entry's rows (the caller sizes one slab for either pass); the kernel's own residency is no smaller than the dense one's
    const int grid = rs_cnn_sized_slab_rows(num_samples, map_side, agent >= 0 ? 6 : 4);
    if (slab_rows < grid) return RS_ERR_INVALID_ARG;
    SzIn in{maps, cells, pcells, num_agents, agent, map_side, map_side / 2, tiles(map_side), (long long)num_samples};
    hipStream_t s = (hipStream_t)stream;
    if (agent >= 0) hipLaunchKernelGGL(rs_sized_trunk_bwd_occ<6>, dim3(grid), dim3(NT), 0, s, in, w2, da2, relu_mask, p1, amax, flags, slab);
    else hipLaunchKernelGGL(rs_sized_trunk_bwd_occ<4>, dim3(grid), dim3(NT), 0, s, in, w2, da2, relu_mask, p1, amax, flags, slab);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

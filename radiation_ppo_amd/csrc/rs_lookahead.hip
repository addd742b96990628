// rs_lookahead.hip -- the env look-ahead (rs_peek: RadSearch.FIM_step, rad_search_env.py:1768-1799, for every agent and all eight
// moves, with a measurement at each candidate) and the policy round of the gradient-search controller on top of it
// (rs_gs_eval_step: GradSearch.step, algos/test_environment/eval/core.py:636-653).  Both kernels run rs_lookahead_lane
// (rs_lookahead.hpp), one lane per (env, agent, move), one-wave workgroups of eight (env, agent) pairs; neither writes env state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_action.hpp"
#include "rs_handle.hpp"
#include "rs_lookahead.hpp"

namespace {

// which (env, agent, move) this lane serves; pair = n * A + a indexes every [N][A] array
struct PeekLane {
    long long pair;
    int n, a, k;
    bool active;
    __device__ __forceinline__ PeekLane(const RsParams& P) {
        const int lane = threadIdx.x & 63;
        k = lane & (RS_PEEK_MOVES - 1);
        pair = (long long)blockIdx.x * RS_PEEK_PAIRS + (lane >> 3);
        active = pair < (long long)P.N * P.A;
        n = active ? (int)(pair / P.A) : 0;
        a = active ? (int)(pair - (long long)n * P.A) : 0;
    }
};

template <bool HAS_OBS>
__global__ void __launch_bounds__(64) rs_peek_kernel(RsParams P, const int32_t* __restrict__ from_xy, int32_t* __restrict__ xy,
                                                     uint8_t* __restrict__ moved, double* __restrict__ lam, int64_t* __restrict__ meas) {
    __shared__ int lds_geo[HAS_OBS ? RS_MAX_VERT * RS_PEEK_PAIRS : 1];
    const PeekLane L(P);
    RsGeo g{lds_geo, 0, 0, 0};
    if (HAS_OBS) {
        rs_peek_load_geo(P, L.n, L.active, lds_geo, g);
        __syncthreads();
    }
    if (!L.active) return;
    const size_t ia = (size_t)L.a * P.N + L.n;
    const int x = from_xy ? from_xy[2 * L.pair] : P.ax[ia], y = from_xy ? from_xy[2 * L.pair + 1] : P.ay[ia];
    const RsPeek r = rs_lookahead_lane<HAS_OBS>(P, g, L.n, L.a, L.k, x, y);
    const size_t o = (size_t)L.pair * RS_PEEK_MOVES + L.k;
    xy[2 * o] = r.x; xy[2 * o + 1] = r.y;
    moved[o] = r.moved ? 1 : 0;
    if (lam) lam[o] = r.lam;
    if (meas) meas[o] = r.meas;
}

// GradSearch.step (core.py:636-653): grad[k] = (meas_k - meas_now) * 0.01 * (1 / q) in float64, rounded once to the float32 tensor
// (:644), 0 for a move that did not take place (:641-642; the reference compares observation coordinates, we use `moved`: the two
// agree except under coord_noise, where the comparison of noisy coordinates means nothing); Categorical(softmax(grad)).sample()
// (:649-653) is rs_draw_action's inverse-CDF draw from the env's own uniform.  The pair's eight gradients are gathered with
// shuffles; every lane of the pair draws (the same action), lane k = 0 stores it.  A finished lane looks nowhere and idles.
template <bool HAS_OBS>
__global__ void __launch_bounds__(64) rs_gs_eval_step_kernel(RsParams P, const float* __restrict__ obs, double q_rec,
                                                             const float* __restrict__ u, const uint8_t* __restrict__ alive,
                                                             int8_t* __restrict__ act8, float* __restrict__ grad_out) {
    __shared__ int lds_geo[HAS_OBS ? RS_MAX_VERT * RS_PEEK_PAIRS : 1];
    const PeekLane L(P);
    const bool live = L.active && alive[L.n] != 0;
    RsGeo g{lds_geo, 0, 0, 0};
    if (HAS_OBS) {
        rs_peek_load_geo(P, L.n, live, lds_geo, g);
        __syncthreads();
    }
    float gk = 0.0f;
    if (live) {
        const size_t ia = (size_t)L.a * P.N + L.n;
        const RsPeek r = rs_lookahead_lane<HAS_OBS>(P, g, L.n, L.a, L.k, P.ax[ia], P.ay[ia]);
        if (r.moved) gk = (float)(((double)r.meas - (double)obs[(size_t)L.pair * RS_OBS_DIM]) * 0.01 * q_rec);
    }
    const int lane = threadIdx.x & 63;
    float gr[RS_PEEK_MOVES];
#pragma unroll
    for (int j = 0; j < RS_PEEK_MOVES; ++j) gr[j] = __shfl(gk, (lane & ~(RS_PEEK_MOVES - 1)) + j);
    int act;
    float lp;
    rs_draw_action<8, 8>(gr, L.active ? u[L.pair] : 0.0f, act, lp);
    if (L.active) {
        if (grad_out) grad_out[(size_t)L.pair * RS_PEEK_MOVES + L.k] = gk;
        if (L.k == 0) act8[L.pair] = live ? (int8_t)act : (int8_t)RS_IDLE;
    }
}

}  // namespace

extern "C" {

int rs_peek(rs_handle* h, const int32_t* from_xy, int32_t* xy, uint8_t* moved, double* lam, int64_t* meas, rs_stream_t stream) {
    if (!h || !xy || !moved) return RS_ERR_INVALID_ARG;
    const RsParams& P = h->P;
    const long long pairs = (long long)P.N * P.A;
    const dim3 grid((unsigned)((pairs + RS_PEEK_PAIRS - 1) / RS_PEEK_PAIRS));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P.obstruction_count != 0) hipLaunchKernelGGL(rs_peek_kernel<true>, grid, dim3(64), 0, s, P, from_xy, xy, moved, lam, meas);
    else hipLaunchKernelGGL(rs_peek_kernel<false>, grid, dim3(64), 0, s, P, from_xy, xy, moved, lam, meas);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_gs_eval_step(rs_handle* h, const float* obs, double q_rec, const float* u, const uint8_t* alive, int8_t* act8, float* grad_out,
                    rs_stream_t stream) {
    if (!h || !obs || !u || !alive || !act8) return RS_ERR_INVALID_ARG;
    const RsParams& P = h->P;
    const long long pairs = (long long)P.N * P.A;
    const dim3 grid((unsigned)((pairs + RS_PEEK_PAIRS - 1) / RS_PEEK_PAIRS));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P.obstruction_count != 0) hipLaunchKernelGGL(rs_gs_eval_step_kernel<true>, grid, dim3(64), 0, s, P, obs, q_rec, u, alive, act8, grad_out);
    else hipLaunchKernelGGL(rs_gs_eval_step_kernel<false>, grid, dim3(64), 0, s, P, obs, q_rec, u, alive, act8, grad_out);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

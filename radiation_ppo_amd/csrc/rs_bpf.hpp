// rs_bpf.hpp -- lane functions of the bootstrap particle filter (ParticleFilter, algos/test_environment/eval/core.py:528-620) and of
// the RID-FIM controller on top of it (FIC, :655-764): the draws, the measurement model, the Fisher term and the workgroup's
// fixed-order reductions.  Everything is float64 with FP contraction off, so sums of products round as numpy's do.
//
// One workgroup of RS_BPF_THREADS lanes per (env, agent) pair; lane t owns the particles t, t + RS_BPF_THREADS, ... in every phase, so
// a lane reads back only what it wrote itself and the phases need a barrier only around a reduction, the resampler and the gather.
//
// Two rules the reference leaves to IEEE accidents (include/radsearch.h says the same):
//   - in renyi_div (:696-701) a candidate reading z whose p_z is 0 contributes 0; the reference computes 0 * (-inf + inf) = nan there;
//   - two moves with the same candidate position give bit-equal J: every move runs one code path with one reduction order.
#pragma once
#include "rs_device.hpp"

#define RS_BPF_THREADS 256
#define RS_BPF_WAVES (RS_BPF_THREADS / RS_WAVE)
#define RS_BPF_ZCHUNK 16           // candidate readings between two directly evaluated pmf values

// ---- draws: key (seed, global env id), counter (slot, step, episode, RS_STREAM_BPF + agent) -- the step and episode words of
// rs_action_uniforms and rs_peek.  Slots 2 p, 2 p + 1: particle p; slot 2 NP + k: the resampler's uniform k.
struct RsBpfKey { uint32_t k0, k1, t, episode, stream; };
__device__ __forceinline__ RsBpfKey rs_bpf_key(const RsParams& P, int n, int a) {
    return RsBpfKey{P.seed, P.env_id_base + (uint32_t)n, P.tstep[n], P.episode[n] - 1u, RS_STREAM_BPF + (uint32_t)a};
}
__device__ __forceinline__ u32x4 rs_bpf_block(const RsBpfKey& K, uint32_t slot) {
    return philox4x32_10(slot, K.t, K.episode, K.stream, K.k0, K.k1);
}
// the prior's uniforms of particle p (rng.uniform, core.py:556-557): intensity, x, y
__device__ __forceinline__ void rs_bpf_prior_u(const RsBpfKey& K, uint32_t p, double& uI, double& ux, double& uy) {
    const u32x4 o = rs_bpf_block(K, 2u * p), q = rs_bpf_block(K, 2u * p + 1u);
    uI = u53(o.x, o.y); ux = u53(o.z, o.w); uy = u53(q.x, q.y);
}
// the process model's standard normals of particle p (rng.normal, core.py:563): Box-Muller in float64, as rs_coord_noise
__device__ __forceinline__ void rs_bpf_normals(const RsBpfKey& K, uint32_t p, double& zI, double& zx, double& zy) {
    const u32x4 o = rs_bpf_block(K, 2u * p), q = rs_bpf_block(K, 2u * p + 1u);
    const double r0 = sqrt(-2.0 * log(1.0 - u53(o.x, o.y))), r1 = sqrt(-2.0 * log(1.0 - u53(q.x, q.y)));
    double sn, cs;
    sincos(6.283185307179586 * u53(o.z, o.w), &sn, &cs);
    zI = r0 * cs; zx = r0 * sn;
    zy = r1 * cos(6.283185307179586 * u53(q.z, q.w));
}
// the resampler's uniform k of NP - 1 (rng.uniform(size=nPart - 1), core.py:574)
__device__ __forceinline__ double rs_bpf_resample_u(const RsBpfKey& K, uint32_t np, uint32_t k) {
    const u32x4 o = rs_bpf_block(K, 2u * np + k);
    return u53(o.x, o.y);
}

// ---- reductions over the workgroup, the same order on every call: butterfly inside a wave (every lane ends with the same bits),
// then the waves' values in wave order.  red: RS_BPF_WAVES doubles of LDS; every lane of the workgroup calls.
__device__ __forceinline__ double rs_bpf_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double rs_bpf_block_sum(double v, double* red) {
    v = rs_bpf_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int i = 1; i < RS_BPF_WAVES; ++i) r += red[i];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double rs_bpf_block_max(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int i = 1; i < RS_BPF_WAVES; ++i) r = fmax(r, red[i]);
    __syncthreads();
    return r;
}

// measModel (core.py:594-596) of one particle for a detector at (dx, dy): np.square(np.linalg.norm(.)) takes the root and squares it
__device__ __forceinline__ double rs_bpf_rate(double I, double x, double y, double detx, double dety, double bkg) {
    const double ex = x - detx, ey = y - dety;
    const double nr = sqrt(ex * ex + ey * ey);
    return rint(I * 1e4 / (nr * nr)) + bkg;
}
// poisson._logpmf(k, lam) = xlogy(k, lam) - gamln(k + 1) - lam (core.py:606); lgk = lgamma(k + 1)
__device__ __forceinline__ double rs_bpf_logpmf(double k, double lgk, double lam) {
    const double xl = (k == 0.0) ? 0.0 : k * log(lam);
    return (xl - lgk) - lam;
}
// one particle's term of trace(particle_FIM @ diag(1e10, 1, 1)) (core.py:686-694), before its weight
__device__ __forceinline__ double rs_bpf_fisher_term(double I, double x, double y, double detx, double dety, double bkg) {
    const double I4 = I * 1e4;
    const double ex = detx - x, ey = dety - y;
    const double den = ex * ex + ey * ey;
    const double f = I4 / (den * den);
    const double g0 = 1.0 / den, g1 = (2.0 * ex) * f, g2 = (2.0 * ey) * f;
    const double s = 1.0 / (I4 / den + bkg);
    return ((g0 * g0 * s) * 1e10 + g1 * g1 * s) + g2 * g2 * s;
}

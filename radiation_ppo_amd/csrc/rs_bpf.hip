// rs_bpf.hip -- the bootstrap particle filter (rs_bpf_track: ParticleFilter.track, algos/test_environment/eval/core.py:554-591, with
// the SSP resampler ssp, :767-799) and the RID-FIM controller's policy round (rs_ridfim_eval_step: FIC.optim_action with L = 1,
// :703-764) for every (env, agent) pair, the particles' 3 x 3 Fisher information matrix (rs_bpf_fim: FIC.particle_FIM, :686-694, and
// the initial bound of test_policy.py:127-135) and the test-facing rs_bpf_draws.  One workgroup of RS_BPF_THREADS lanes per pair
// (rs_bpf.hpp); the candidate positions of the eight moves are rs_peek's lane function (rs_lookahead.hpp).  No kernel writes env
// state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_bpf.hpp"
#include "rs_handle.hpp"
#include "rs_lookahead.hpp"

// the two opaque objects of the header
struct rs_bpf_params {
    int32_t num_particles;
    double sigma_xy, sigma_I, thresh;
    double intensity[2], coord[2];
    double alpha, fim_thresh;
    int32_t interval[2];
};
struct rs_bpf_state {
    int32_t num_pairs;
    double *xp, *w, *logw, *est, *neff;
    uint8_t* rdiv;
    uint32_t* flags;
    void* scratch;
    size_t scratch_bytes;
};

namespace {

#define RS_SSP_CHUNK 512           // chain steps staged in LDS at a time

// the pair's slices of the caller's state
struct BpfArgs {
    int NP;
    double sigma_xy, sigma_I, thresh, i_lo, i_hi, c_lo, c_hi, alpha, fim_thresh;
    int i0, i1;
    double *xp, *w, *logw, *est, *neff;
    uint8_t* rdiv;
    uint32_t* flags;
    double* xp2;                   // [pairs][3][NP]
    uint32_t* children;            // [pairs][NP]
};

__host__ size_t bpf_children_offset(long long pairs, int NP) { return (size_t)pairs * 3 * (size_t)NP * sizeof(double); }

// logw += logpmf over the lane's particles, then w = exp(logw - max) / sum and sum w^2 (core.py:566-571); returns 1 / sum w^2 rounded
__device__ __forceinline__ double bpf_weigh(const BpfArgs& B, const double* xI, const double* xx, const double* xy, double* w, double* lw,
                                            bool from_zero, double k, double lgk, double detx, double dety, double bkg, double* red) {
    const int NP = B.NP;
    double m = -INFINITY;
    for (int p = threadIdx.x; p < NP; p += RS_BPF_THREADS) {
        const double ll = rs_bpf_logpmf(k, lgk, rs_bpf_rate(xI[p], xx[p], xy[p], detx, dety, bkg));
        const double l = (from_zero ? 0.0 : lw[p]) + ll;
        lw[p] = l;
        m = fmax(m, l);
    }
    m = rs_bpf_block_max(m, red);
    double s = 0.0;
    for (int p = threadIdx.x; p < NP; p += RS_BPF_THREADS) {
        const double e = exp(lw[p] - m);
        w[p] = e;
        s += e;
    }
    s = rs_bpf_block_sum(s, red);
    double q = 0.0;
    for (int p = threadIdx.x; p < NP; p += RS_BPF_THREADS) {
        const double wn = w[p] / s;
        w[p] = wn;
        q += wn * wn;
    }
    q = rs_bpf_block_sum(q, red);
    return rint(1.0 / q);
}

__global__ void __launch_bounds__(RS_BPF_THREADS) rs_bpf_track_kernel(RsParams P, BpfArgs B, const float* __restrict__ obs,
                                                                       const uint8_t* __restrict__ alive, int first) {
    __shared__ double red[RS_BPF_WAVES];
    __shared__ double c_xi[RS_SSP_CHUNK], c_u[RS_SSP_CHUNK];
    __shared__ int c_fl[RS_SSP_CHUNK];
    __shared__ int seg_sum[RS_BPF_THREADS];
    __shared__ int ssp_ok;
    const long long pair = blockIdx.x;
    const int n = (int)(pair / P.A), a = (int)(pair - (long long)n * P.A);
    if (alive[n] == 0) return;                               // the whole workgroup: a finished lane's state is left alone
    const int NP = B.NP, tid = threadIdx.x;
    double* xI = B.xp + (size_t)pair * 3 * NP;
    double* xx = xI + NP;
    double* xy = xx + NP;
    double* w = B.w + (size_t)pair * NP;
    double* lw = B.logw + (size_t)pair * NP;
    const RsBpfKey K = rs_bpf_key(P, n, a);
    const size_t ia = (size_t)a * P.N + n;
    const double detx = (double)P.ax[ia], dety = (double)P.ay[ia], bkg = (double)P.bkg[n];
    const double k = (double)obs[(size_t)pair * RS_OBS_DIM];
    const double lgk = lgamma(k + 1.0);
    uint32_t flags = B.flags[pair] & RS_BPF_ERR_SSP;

    if (first) {                                             // core.py:556-561
        const double lw0 = log(1.0 / (double)NP);
        for (int p = tid; p < NP; p += RS_BPF_THREADS) {
            double uI, ux, uy;
            rs_bpf_prior_u(K, (uint32_t)p, uI, ux, uy);
            xI[p] = B.i_lo + (B.i_hi - B.i_lo) * uI;
            xx[p] = B.c_lo + (B.c_hi - B.c_lo) * ux;
            xy[p] = B.c_lo + (B.c_hi - B.c_lo) * uy;
            lw[p] = lw0;
        }
        if (tid == 0) B.rdiv[pair] = 1;
    } else {                                                 // processModel, core.py:598-601
        for (int p = tid; p < NP; p += RS_BPF_THREADS) {
            double zI, zx, zy;
            rs_bpf_normals(K, (uint32_t)p, zI, zx, zy);
            xx[p] = xx[p] + B.sigma_xy * zx;
            xy[p] = xy[p] + B.sigma_xy * zy;
            xI[p] = fmax(xI[p] + B.sigma_I * zI, 0.0);
        }
    }
    // nEff is appended before the resampling and not again (core.py:571): the value reported is this one
    const double neff = bpf_weigh(B, xI, xx, xy, w, lw, false, k, lgk, detx, dety, bkg, red);

    if (neff < B.thresh * (double)NP) {                      // core.py:573-579
        flags |= RS_BPF_RESAMPLED;
        uint32_t* cnt = B.children + (size_t)pair * NP;
        double* g0 = B.xp2 + (size_t)pair * 3 * NP;
        // ssp (core.py:767-799).  Only xi[i] and xi[j] are carried and xi[k + 2] is read in order, so lane 0 keeps the two carried
        // entries (xi and child count) in registers and writes a child count when its index leaves the chain; the workgroup stages
        // xi[k + 2], floor(M W)[k + 2] and u[k] of RS_SSP_CHUNK steps in LDS ahead of it.
        int i = 0, j = 1, ci = 0, cj = 0, total = 0;
        double xi_i = 0.0, xi_j = 0.0;
        if (tid == 0) {
            const double m0 = (double)NP * w[0], m1 = (double)NP * w[1];
            const double f0 = floor(m0), f1 = floor(m1);
            xi_i = m0 - f0; xi_j = m1 - f1; ci = (int)f0; cj = (int)f1; total = ci + cj;
        }
        __syncthreads();                                     // every lane's w is in memory before another lane reads it
        for (int kb = 0; kb < NP - 1; kb += RS_SSP_CHUNK) {
            for (int t = tid; t < RS_SSP_CHUNK; t += RS_BPF_THREADS) {
                const int ks = kb + t, e = ks + 2;
                c_u[t] = ks < NP - 1 ? rs_bpf_resample_u(K, (uint32_t)NP, (uint32_t)ks) : 0.0;
                const double mw = e < NP ? (double)NP * w[e] : 0.0;
                const double fl = floor(mw);
                c_xi[t] = mw - fl; c_fl[t] = (int)fl;
            }
            __syncthreads();
            if (tid == 0) {
                const int kend = min(RS_SSP_CHUNK, NP - 1 - kb);
                for (int t = 0; t < kend; ++t) {
                    double delta_i = fmin(xi_j, 1.0 - xi_i);           // increase i, decrease j
                    const double delta_j = fmin(xi_i, 1.0 - xi_j);     // the opposite
                    const double sum_delta = delta_i + delta_j;
                    const double pj = sum_delta > 0.0 ? delta_i / sum_delta : 0.0;
                    if (c_u[t] < pj) {                                 // swap i, j, so that we always increase i
                        const int ti = i; i = j; j = ti;
                        const int tc = ci; ci = cj; cj = tc;
                        const double tx = xi_i; xi_i = xi_j; xi_j = tx;
                        delta_i = delta_j;
                    }
                    const int e = kb + t + 2;                          // the index that enters the chain; e == NP at the last step
                    if (xi_j < 1.0 - xi_i) {
                        xi_i += delta_i;
                        cnt[j] = (uint32_t)cj;
                        j = e; xi_j = c_xi[t]; cj = c_fl[t];
                    } else {
                        xi_j -= delta_i;
                        ci += 1; total += 1;
                        cnt[i] = (uint32_t)ci;
                        i = e; xi_i = c_xi[t]; ci = c_fl[t];
                    }
                    total += c_fl[t];                                  // 0 for e == NP
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            // due to round-off error accumulation, we may be missing one particle (core.py:791-795)
            const bool last_is_i = (j == NP);
            const int last = last_is_i ? i : j;
            int cl = last_is_i ? ci : cj;
            const double xl = last_is_i ? xi_i : xi_j;
            if (total == NP - 1 && xl > 0.99) { cl += 1; total += 1; }
            cnt[last] = (uint32_t)cl;
            ssp_ok = (total == NP) ? 1 : 0;
        }
        __syncthreads();
        if (ssp_ok) {
            // np.arange(N).repeat(nr_children): contiguous segments of parents per lane, an exclusive scan of the segments' sums,
            // every parent's copies to the second buffer, then back
            const int seg = (NP + RS_BPF_THREADS - 1) / RS_BPF_THREADS;
            const int q0 = min(tid * seg, NP), q1 = min(q0 + seg, NP);
            int mine = 0;
            for (int q = q0; q < q1; ++q) mine += (int)cnt[q];
            seg_sum[tid] = mine;
            __syncthreads();
            int off = 0;
            for (int t = 0; t < tid; ++t) off += seg_sum[t];
            for (int q = q0; q < q1; ++q) {
                const int c = (int)cnt[q];
                const double vI = xI[q], vx = xx[q], vy = xy[q];
                for (int r = 0; r < c; ++r) {
                    const int d = off + r;
                    if (d < NP) { g0[d] = vI; g0[NP + d] = vx; g0[2 * NP + d] = vy; }
                }
                off += c;
            }
            __syncthreads();
            for (int p = tid; p < NP; p += RS_BPF_THREADS) { xI[p] = g0[p]; xx[p] = g0[NP + p]; xy[p] = g0[2 * NP + p]; }
        } else {
            flags |= RS_BPF_ERR_SSP;
        }
        bpf_weigh(B, xI, xx, xy, w, lw, true, k, lgk, detx, dety, bkg, red);
    }
    // update_measures (core.py:613-615) and wp = log(wp) (:588)
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    for (int p = tid; p < NP; p += RS_BPF_THREADS) {
        const double wv = w[p];
        e0 += wv * xI[p]; e1 += wv * xx[p]; e2 += wv * xy[p];
        lw[p] = log(wv);
    }
    e0 = rs_bpf_block_sum(e0, red); e1 = rs_bpf_block_sum(e1, red); e2 = rs_bpf_block_sum(e2, red);
    if (tid == 0) {
        B.est[3 * pair] = e0; B.est[3 * pair + 1] = e1; B.est[3 * pair + 2] = e2;
        B.neff[pair] = neff;
        B.flags[pair] = flags;
    }
}

// FIC.optim_action with L = 1 (core.py:703-764) for one pair
template <bool HAS_OBS>
__global__ void __launch_bounds__(RS_BPF_THREADS) rs_ridfim_eval_step_kernel(RsParams P, BpfArgs B, const float* __restrict__ obs,
                                                                              const uint8_t* __restrict__ alive, int8_t* __restrict__ act8,
                                                                              double* __restrict__ J_out, double* __restrict__ Jf_out) {
    __shared__ int lds_geo[HAS_OBS ? RS_MAX_VERT * RS_PEEK_PAIRS : 1];
    __shared__ int cand[RS_PEEK_MOVES][2];
    __shared__ double red[RS_BPF_WAVES];
    __shared__ double red32[RS_BPF_WAVES][2 * RS_BPF_ZCHUNK];
    __shared__ double rz[RS_BPF_MAX_WINDOW + RS_BPF_ZCHUNK], zpa[RS_BPF_MAX_WINDOW + RS_BPF_ZCHUNK];
    __shared__ double lgz[RS_BPF_MAX_WINDOW / RS_BPF_ZCHUNK + 1];
    __shared__ double jpart[RS_BPF_ZCHUNK];
    __shared__ double Jk[RS_PEEK_MOVES], Jf[RS_PEEK_MOVES];
    const long long pair = blockIdx.x;
    const int n = (int)(pair / P.A), a = (int)(pair - (long long)n * P.A);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (alive[n] == 0) {                                     // the whole workgroup
        if (tid == 0) act8[pair] = (int8_t)RS_IDLE;
        return;
    }
    const int NP = B.NP;
    const double* xI = B.xp + (size_t)pair * 3 * NP;
    const double* xx = xI + NP;
    const double* xy = xx + NP;
    const double* w = B.w + (size_t)pair * NP;
    double* s_lam = B.xp2 + (size_t)pair * 3 * NP;           // this move's rate, its logarithm and its alpha-th power, per particle
    double* s_log = s_lam + NP;
    double* s_pow = s_log + NP;
    const double bkg = (double)P.bkg[n], alpha = B.alpha;
    const bool renyi = B.rdiv[pair] == 1;

    // the eight candidate positions: the position part of rs_peek's lane function (no path, rate or measurement draw), by the first
    // eight lanes (pair slot 0 of the look-ahead's wave layout)
    RsGeo g{lds_geo, 0, 0, 0};
    if (HAS_OBS) {
        if (wave == 0) rs_peek_load_geo(P, n, true, lds_geo, g);
        __syncthreads();
    }
    if (tid < RS_PEEK_MOVES) {
        const size_t ia = (size_t)a * P.N + n;
        int cx, cy;
        rs_lookahead_xy<HAS_OBS>(P, g, tid, P.ax[ia], P.ay[ia], cx, cy);
        cand[tid][0] = cx; cand[tid][1] = cy;
    }
    // the candidate readings z_t = zlo + t, t < Z (core.py:708), and what depends on z alone
    const double x0 = (double)obs[(size_t)pair * RS_OBS_DIM];
    const double zlo = fmax(x0 - (double)B.i0, 1.0), zhi = x0 + (double)B.i1;
    const int Z = (renyi && zhi > zlo) ? min((int)ceil(zhi - zlo), RS_BPF_MAX_WINDOW) : 0;
    const int chunks = (Z + RS_BPF_ZCHUNK - 1) / RS_BPF_ZCHUNK;
    for (int t = tid; t < chunks * RS_BPF_ZCHUNK; t += RS_BPF_THREADS) {
        const double z1 = zlo + (double)t + 1.0;
        rz[t] = 1.0 / z1;                                    // pmf(z + 1) = pmf(z) lam / (z + 1)
        zpa[t] = exp(-alpha * log(z1));                      // (z + 1)^-alpha
    }
    for (int c = tid; c < chunks; c += RS_BPF_THREADS) lgz[c] = lgamma(zlo + (double)(c * RS_BPF_ZCHUNK) + 1.0);
    __syncthreads();

    for (int mv = 0; mv < RS_PEEK_MOVES; ++mv) {
        const double cx = (double)cand[mv][0], cy = (double)cand[mv][1];
        double fa = 0.0;
        for (int p = tid; p < NP; p += RS_BPF_THREADS) {
            const double I = xI[p], x = xx[p], y = xy[p];
            fa += rs_bpf_fisher_term(I, x, y, cx, cy, bkg) * w[p];
            if (renyi) {
                const double lam = rs_bpf_rate(I, x, y, cx, cy, bkg), ll = log(lam);
                s_lam[p] = lam; s_log[p] = ll; s_pow[p] = exp(alpha * ll);
            }
        }
        const double jf = rs_bpf_block_sum(fa, red);
        double jacc = 0.0;                                   // lanes 0..15: the terms of the readings t = lane (mod 16), in chunk order
        for (int c = 0; c < chunks; ++c) {
            const int t0 = c * RS_BPF_ZCHUNK;
            const double z0 = zlo + (double)t0, lg0 = lgz[c];
            double az[RS_BPF_ZCHUNK], aa[RS_BPF_ZCHUNK];
#pragma unroll
            for (int q = 0; q < RS_BPF_ZCHUNK; ++q) { az[q] = 0.0; aa[q] = 0.0; }
            for (int p = tid; p < NP; p += RS_BPF_THREADS) {
                const double lam = s_lam[p], ll = s_log[p], la = s_pow[p], wv = w[p];
                const double e0 = (z0 * ll - lg0) - lam;     // poisson._pmf: exp(xlogy(z, lam) - gamln(z + 1) - lam), z >= 1
                const double pm = exp(e0);
                double wpm = wv * pm, wpa = wv * (pm > 0.0 ? exp(alpha * e0) : 0.0);     // pmf^alpha of an underflowed pmf is 0
                az[0] += wpm; aa[0] += wpa;
#pragma unroll
                for (int q = 1; q < RS_BPF_ZCHUNK; ++q) {
                    wpm *= lam * rz[t0 + q - 1];
                    wpa *= la * zpa[t0 + q - 1];
                    az[q] += wpm; aa[q] += wpa;
                }
            }
#pragma unroll
            for (int q = 0; q < RS_BPF_ZCHUNK; ++q) {
                const double sz = rs_bpf_wave_sum(az[q]), sa = rs_bpf_wave_sum(aa[q]);
                if (lane == 0) { red32[wave][q] = sz; red32[wave][RS_BPF_ZCHUNK + q] = sa; }
            }
            __syncthreads();
            if (tid < RS_BPF_ZCHUNK && t0 + tid < Z) {
                double pz = red32[0][tid], pza = red32[0][RS_BPF_ZCHUNK + tid];
#pragma unroll
                for (int v = 1; v < RS_BPF_WAVES; ++v) { pz += red32[v][tid]; pza += red32[v][RS_BPF_ZCHUNK + tid]; }
                if (pz > 0.0) jacc += pz * (log(pza) - alpha * log(pz));         // p_z == 0 contributes 0 (rs_bpf.hpp)
            }
            __syncthreads();
        }
        if (tid < RS_BPF_ZCHUNK) jpart[tid] = jacc;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
#pragma unroll
            for (int q = 0; q < RS_BPF_ZCHUNK; ++q) sum += jpart[q];
            Jf[mv] = jf;
            Jk[mv] = renyi ? (1.0 / (alpha - 1.0)) * sum : jf;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int best = 0;                                        // np.argmax: the first nan if there is one, else the first index of the maximum
        for (int mv = 1; mv < RS_PEEK_MOVES; ++mv)
            if (!(Jk[best] != Jk[best]) && (Jk[mv] != Jk[mv] || Jk[mv] > Jk[best])) best = mv;
        if (renyi && Jk[best] > B.fim_thresh) B.rdiv[pair] = 0;                  // core.py:758-759
        act8[pair] = (int8_t)best;
    }
    if (tid < RS_PEEK_MOVES) {
        if (J_out) J_out[(size_t)pair * RS_PEEK_MOVES + tid] = Jk[tid];
        if (Jf_out) Jf_out[(size_t)pair * RS_PEEK_MOVES + tid] = Jf[tid];
    }
}

__global__ void __launch_bounds__(RS_BPF_THREADS) rs_bpf_draws_kernel(RsParams P, int NP, double* __restrict__ prior_u,
                                                                       double* __restrict__ normals, double* __restrict__ resample_u) {
    const long long pair = blockIdx.x;
    const int n = (int)(pair / P.A), a = (int)(pair - (long long)n * P.A);
    const RsBpfKey K = rs_bpf_key(P, n, a);
    for (int p = threadIdx.x; p < NP; p += RS_BPF_THREADS) {
        const size_t o = (size_t)pair * 3 * NP + p;
        if (prior_u) {
            double uI, ux, uy;
            rs_bpf_prior_u(K, (uint32_t)p, uI, ux, uy);
            prior_u[o] = uI; prior_u[o + NP] = ux; prior_u[o + 2 * (size_t)NP] = uy;
        }
        if (normals) {
            double zI, zx, zy;
            rs_bpf_normals(K, (uint32_t)p, zI, zx, zy);
            normals[o] = zI; normals[o + NP] = zx; normals[o + 2 * (size_t)NP] = zy;
        }
        if (resample_u && p < NP - 1) resample_u[(size_t)pair * (NP - 1) + p] = rs_bpf_resample_u(K, (uint32_t)NP, (uint32_t)p);
    }
}

// FIC.particle_FIM (core.py:686-694) of one pair at (detx, dety): F[i][j] = sum_p w_p ((g_i g_j) s) c_j, the column scale c = J @ scale.
// PRIOR: the particles are the prior's, regenerated from the draws rs_bpf_track(first = 1) consumes at the env's present step, with
// weights 1 / NP (test_policy.py:127-135); nothing is read from the state.  A particle exactly at the position gives inf / nan, as numpy.
template <bool PRIOR>
__global__ void __launch_bounds__(RS_BPF_THREADS) rs_bpf_fim_kernel(RsParams P, BpfArgs B, const uint8_t* __restrict__ alive,
                                                                     const double* __restrict__ pos, double c0, double c1, double c2,
                                                                     double* __restrict__ F, double* __restrict__ trace) {
    __shared__ double red[RS_BPF_WAVES];
    const long long pair = blockIdx.x;
    const int n = (int)(pair / P.A), a = (int)(pair - (long long)n * P.A);
    if (alive[n] == 0) return;                               // the whole workgroup: none of a finished lane's outputs is written
    const int NP = B.NP, tid = threadIdx.x;
    const double* xI = B.xp + (size_t)pair * 3 * NP;
    const double* xx = xI + NP;
    const double* xy = xx + NP;
    const double* w = B.w + (size_t)pair * NP;
    const size_t ia = (size_t)a * P.N + n;
    const double detx = pos ? pos[2 * pair] : (double)P.ax[ia], dety = pos ? pos[2 * pair + 1] : (double)P.ay[ia];
    const double bkg = (double)P.bkg[n], w0 = 1.0 / (double)NP;
    const RsBpfKey K = rs_bpf_key(P, n, a);
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[q] = 0.0;
    for (int p = tid; p < NP; p += RS_BPF_THREADS) {
        double I, x, y, wv;
        if (PRIOR) {
            double uI, ux, uy;
            rs_bpf_prior_u(K, (uint32_t)p, uI, ux, uy);
            I = B.i_lo + (B.i_hi - B.i_lo) * uI;
            x = B.c_lo + (B.c_hi - B.c_lo) * ux;
            y = B.c_lo + (B.c_hi - B.c_lo) * uy;
            wv = w0;
        } else {
            I = xI[p]; x = xx[p]; y = xy[p]; wv = w[p];
        }
        const double I4 = I * 1e4;
        const double ex = detx - x, ey = dety - y;
        const double den = ex * ex + ey * ey;
        const double f = I4 / (den * den);
        const double g[3] = {1.0 / den, (2.0 * ex) * f, (2.0 * ey) * f};
        const double s = 1.0 / (I4 / den + bkg);
        const double c[3] = {c0, c1, c2};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 * i + j] += (((g[i] * g[j]) * s) * c[j]) * wv;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[q] = rs_bpf_block_sum(acc[q], red);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 9; ++q) F[(size_t)pair * 9 + q] = acc[q];
        if (trace) trace[pair] = (acc[0] + acc[4]) + acc[8];
    }
}

// the refusals of both entries and the kernels' argument block; false: refuse
bool bpf_args(const rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, BpfArgs& B) {
    if (!h || !p || !s) return false;
    const long long pairs = (long long)h->P.N * h->P.A;
    if (s->num_pairs != pairs) return false;
    if (s->scratch_bytes < rs_bpf_scratch_bytes(s->num_pairs, p->num_particles)) return false;
    B.NP = p->num_particles;
    B.sigma_xy = p->sigma_xy; B.sigma_I = p->sigma_I; B.thresh = p->thresh;
    B.i_lo = p->intensity[0]; B.i_hi = p->intensity[1]; B.c_lo = p->coord[0]; B.c_hi = p->coord[1];
    B.alpha = p->alpha; B.fim_thresh = p->fim_thresh; B.i0 = p->interval[0]; B.i1 = p->interval[1];
    B.xp = s->xp; B.w = s->w; B.logw = s->logw; B.est = s->est; B.neff = s->neff; B.rdiv = s->rdiv; B.flags = s->flags;
    B.xp2 = static_cast<double*>(s->scratch);
    B.children = reinterpret_cast<uint32_t*>(static_cast<char*>(s->scratch) + bpf_children_offset(pairs, B.NP));
    return true;
}

}  // namespace

extern "C" {

int rs_bpf_params_create(int32_t num_particles, double sigma_xy, double sigma_I, double thresh, const double* intensity, const double* coord,
                         double alpha, double fim_thresh, const int32_t* interval, rs_bpf_params** out) {
    if (!intensity || !coord || !interval || !out || num_particles < 2) return RS_ERR_INVALID_ARG;
    if (!(sigma_xy >= 0.0) || !(sigma_I >= 0.0) || !(thresh >= 0.0)) return RS_ERR_INVALID_ARG;
    if (!(intensity[1] >= intensity[0]) || !(coord[1] >= coord[0])) return RS_ERR_INVALID_ARG;
    if (alpha == 1.0 || !(alpha == alpha) || !(fim_thresh == fim_thresh)) return RS_ERR_INVALID_ARG;
    if (interval[0] < 0 || interval[1] < 0 || (long long)interval[0] + interval[1] > RS_BPF_MAX_WINDOW) return RS_ERR_INVALID_ARG;
    *out = new rs_bpf_params{num_particles, sigma_xy, sigma_I, thresh, {intensity[0], intensity[1]}, {coord[0], coord[1]}, alpha, fim_thresh,
                             {interval[0], interval[1]}};
    return RS_OK;
}

void rs_bpf_params_destroy(rs_bpf_params* p) { delete p; }

int rs_bpf_state_create(int32_t num_pairs, double* xp, double* w, double* logw, double* est, double* neff, uint8_t* rdiv, uint32_t* flags,
                        void* scratch, size_t scratch_bytes, rs_bpf_state** out) {
    if (num_pairs < 1 || !xp || !w || !logw || !est || !neff || !rdiv || !flags || !scratch || !out) return RS_ERR_INVALID_ARG;
    *out = new rs_bpf_state{num_pairs, xp, w, logw, est, neff, rdiv, flags, scratch, scratch_bytes};
    return RS_OK;
}

void rs_bpf_state_destroy(rs_bpf_state* s) { delete s; }

size_t rs_bpf_scratch_bytes(int32_t num_pairs, int32_t num_particles) {
    if (num_pairs < 1 || num_particles < 2) return 0;
    return bpf_children_offset(num_pairs, num_particles) + (size_t)num_pairs * (size_t)num_particles * sizeof(uint32_t);
}

int rs_bpf_track(rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, const float* obs, const uint8_t* alive, int32_t first,
                 rs_stream_t stream) {
    BpfArgs B;
    if (!obs || !alive || !bpf_args(h, p, s, B)) return RS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rs_bpf_track_kernel, dim3((unsigned)s->num_pairs), dim3(RS_BPF_THREADS), 0, static_cast<hipStream_t>(stream), h->P,
                       B, obs, alive, (int)first);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_ridfim_eval_step(rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, const float* obs, const uint8_t* alive, int8_t* act8,
                        double* J, double* J_fish, rs_stream_t stream) {
    BpfArgs B;
    if (!obs || !alive || !act8 || !bpf_args(h, p, s, B)) return RS_ERR_INVALID_ARG;
    const dim3 grid((unsigned)s->num_pairs);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (h->P.obstruction_count != 0)
        hipLaunchKernelGGL(rs_ridfim_eval_step_kernel<true>, grid, dim3(RS_BPF_THREADS), 0, st, h->P, B, obs, alive, act8, J, J_fish);
    else
        hipLaunchKernelGGL(rs_ridfim_eval_step_kernel<false>, grid, dim3(RS_BPF_THREADS), 0, st, h->P, B, obs, alive, act8, J, J_fish);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_bpf_draws(rs_handle* h, int32_t num_particles, double* prior_u, double* normals, double* resample_u, rs_stream_t stream) {
    if (!h || num_particles < 2) return RS_ERR_INVALID_ARG;
    const long long pairs = (long long)h->P.N * h->P.A;
    hipLaunchKernelGGL(rs_bpf_draws_kernel, dim3((unsigned)pairs), dim3(RS_BPF_THREADS), 0, static_cast<hipStream_t>(stream), h->P,
                       (int)num_particles, prior_u, normals, resample_u);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_bpf_fim(rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, const uint8_t* alive, const double* pos, int32_t prior, double* F,
               double* trace, rs_stream_t stream) {
    BpfArgs B;
    if (!alive || !F || !bpf_args(h, p, s, B)) return RS_ERR_INVALID_ARG;
    const dim3 grid((unsigned)s->num_pairs);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (prior)                                               // scale @ uni_probs (test_policy.py:362-365) from the params' prior box
        hipLaunchKernelGGL(rs_bpf_fim_kernel<true>, grid, dim3(RS_BPF_THREADS), 0, st, h->P, B, alive, pos, 1e10 / (B.i_hi - B.i_lo),
                           1.0 / (B.c_hi - B.c_lo), 1.0 / (B.c_hi - B.c_lo), F, trace);
    else
        hipLaunchKernelGGL(rs_bpf_fim_kernel<false>, grid, dim3(RS_BPF_THREADS), 0, st, h->P, B, alive, pos, 1e10, 1.0, 1.0, F, trace);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

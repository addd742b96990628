// rs_pfgru_sized.hip -- K11's PFGRU location predictor at hidden widths H = 8, 16, .., 64 (a multiple of 8):
// the particle-filter step and its multi-step pass (the reset: rs_draws.hip).  40 particles, 3 inputs, alpha 0.7, tanh and the hid_obs head
// Linear(H, 24)-ReLU-Linear(24, 2)-ReLU stay what the reference fixes (RADTEAM_core.py:1533-1584; PFGRUCell's default width is 64,
// RAD-TEAM's --hid-rec).  The draw contract is K11's: the counter hash of radiation_ppo_amd/pfgru.py keyed by particle * 4096 + unit,
// one hash_normal hash per PAIR of units, one resampling uniform per particle, h0 ~ hash_uniform at reset; the particle sets are
// quad-major [A][N][H / 4][P][4].  K11 (rs_pfgru.hip) still serves 24 units; these kernels also instantiate 24 (tests hold them to K11).
//
// Decomposition (per width: DESIGN.md section 3).  Six (owner, env) sets of 40 particles per 256-thread workgroup, one particle per lane,
// as K11; what couples a set's particles goes through LDS and nine workgroup barriers, every lane reducing a set's 40 values in index
// order (deterministic, independent of which sets share a workgroup, so predictions do not depend on the sharding).  K11 holds a
// particle's units, gates and candidate in registers; at 64 units that is 4 x 64 values, so here only two H-vectors live in a lane:
//   pass 1  r = sigmoid(W_r [h0, x] + b) in 16-column chunks (unrolled): rh = r * h0 in registers (H VGPRs) next to h0 (H VGPRs);
//   pass 2  a RUNTIME loop over 8-unit blocks: z (8 columns, from h0) and [mu | var] (16 columns, from rh) of the block, the block's
//           reparameterisation draws, h1 = (1 - z) n + z h0 with h0 read from the set's LDS tile [40][H + 1], h1 written back into the
//           same tile (the lane's own row: no barrier), the observation logit accumulated unit by unit in K11's order.
// The tile is then the resampling gather's source and the weighted mean's, as in K11.  Weights are workgroup-uniform and stream through
// the scalar unit (rs_sstream.hpp).  Per width: VGPRs / LDS / waves per SIMD the launch bounds are cut for:
//   H 8, 16: 4 waves per SIMD (<= 128 VGPRs)   24, 32: 3 (<= 168)   40 .. 56: 2 (<= 256; LDS 46-61 KB per workgroup)   64: 1 (255 VGPRs)
// hipcc keeps about three H-vectors live across the block loop (h0, rh and the gathered particle); cut for two waves, 64 units spill
// (52 B of scratch).  Exact counts: tests/test_pfgru_sized_resources.py.
//
// Instantiations: rs_pfgru_sized_kernel<H, false> serves the collectors' step (one step per launch) and the pass (up to
// RS_PFGRU_SIZED_PASS_STEPS steps per launch in a runtime loop, the particle set staying in registers in between); <H, true> reads the
// noise and the resampling indices from buffers (the reference's recorded runs: tests/golden/pfgru_sized.npz).
//
// Packed weights of one owner (floats; packer: radiation_ppo_amd/pfgru.py: pack_sized_weights), K = H + 3 inputs [h | x], nb = H / 8:
//   R [K][H] (k-major fc_r) | RB [H] | ZN: nb blocks of [K][24] (columns 0..7 = fc_z of units 8b..8b+7, 8..15 = mu, 16..23 = var of the
//   same units) | ZNB [nb][24] | O [K] | OB [1] | pad to 16 | H0 [H][24] (k-major hid_obs.0) | H0B [24] | H2 [2][24] | H2B [2] | pad to 16
// every region starting at a multiple of 16 floats.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_draws.hpp"
#include "rs_sstream.hpp"

namespace {

constexpr int SP = RS_PFGRU_PARTICLES, SIN = 3;                   // 40 particles, 3 inputs
__host__ __device__ constexpr int r16(int v) { return (v + 15) / 16 * 16; }
struct SLayout {
    int R, RB, ZN, ZNB, O, OB, H0, H0B, H2, H2B, stride;
};
__host__ __device__ constexpr SLayout slayout(int H) {
    const int K = H + SIN, nb = H / 8;
    const int R = 0, RB = r16(R + K * H), ZN = r16(RB + H), ZNB = r16(ZN + nb * K * 24), O = r16(ZNB + nb * 24), OB = O + K,
              H0 = r16(OB + 1), H0B = H0 + H * 24, H2 = H0B + 24, H2B = H2 + 48;
    return SLayout{R, RB, ZN, ZNB, O, OB, H0, H0B, H2, H2B, r16(H2B + 2)};
}
bool width_ok(int H) { return H >= 8 && H <= 64 && H % 8 == 0; }


constexpr int SZ_MAXSTEPS = 16;
#ifndef RS_PFGRU_SIZED_PASS_STEPS
#define RS_PFGRU_SIZED_PASS_STEPS 8        // time steps per launch of rs_pfgru_sized_pass (1 .. 16): scripts/time_pfgru_sized.py
#endif
static_assert(RS_PFGRU_SIZED_PASS_STEPS >= 1 && RS_PFGRU_SIZED_PASS_STEPS <= SZ_MAXSTEPS, "steps per launch");

struct SzArgs {
    const float* w;           // [A][stride]
    const float* obs;         // [N][A][11]
    float* h;                 // [A][N][H / 4][P][4]
    float* p;                 // [A][N][P]
    const int64_t* base;      // [A][N]
    const int64_t* episode;   // [N]
    const int64_t* calls;     // [N] (per step: step_stride apart)
    const uint8_t* mask;      // [N] or null
    float* pred;              // [N][A][2]
    const float* eps_in;      // [A][N][P][H]  } recorded draws (REC only)
    const int32_t* idx_in;    // [A][N][P]     }
    int N, A, carry, steps;
    int Ns[SZ_MAXSTEPS];      // steps > 1: the sets still running at the launch's step s (Ns[s - 1], prefixes of N, descending)
    long long step_stride;
    float alpha, floor_;
};

constexpr int SZ_SETS = 6, SZ_NT = 256;
// LDS of one set (floats): tile [40][H + 1] | cdf 40 x f64 | va [40] | vb [40] | vc [40] | vm [H]; stride 12 (mod 32) banks as K11
__host__ __device__ constexpr int sz_lds_stride(int H) {
    const int b = (SP * (H + 1) + 2 * SP + 3 * SP + H + 3) / 4 * 4;
    return b + ((12 - b % 32) + 32) % 32;
}
__host__ __device__ constexpr int sz_occ(int H) { return H <= 16 ? 4 : (H <= 32 ? 3 : (H <= 56 ? 2 : 1)); }


template <int H, bool REC>
__global__ void __launch_bounds__(SZ_NT, sz_occ(H)) rs_pfgru_sized_kernel(SzArgs a_, int groups) {
    constexpr int K = H + SIN, ROW = H + 1, LS = sz_lds_stride(H);
    constexpr SLayout L = slayout(H);
    constexpr int T_CDF = SP * ROW, T_VA = T_CDF + 2 * SP, T_VB = T_VA + SP, T_VC = T_VB + SP, T_VM = T_VC + SP;
    static_assert(T_VM + H <= LS && T_CDF % 2 == 0 && LS % 4 == 0, "LDS layout of a particle set");
    __shared__ __align__(16) float smem[SZ_SETS * LS];
    const int tid = threadIdx.x;
    const int own = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)groups));
    const int grp = blockIdx.x - own * groups;
    const int set = tid / SP, q = tid - set * SP;                    // set == SZ_SETS: the 16 lanes that carry nothing
    const int n_raw = grp * SZ_SETS + set;
    const bool in_range = set < SZ_SETS && n_raw < a_.N;
    const int n = in_range ? n_raw : a_.N - 1;
    const bool live = in_range && (a_.mask == nullptr || a_.mask[n] != 0);
    if (__syncthreads_or(live ? 1 : 0) == 0) return;
    float* S = smem + (set < SZ_SETS ? set : SZ_SETS - 1) * LS;
    float* tile = S;
    double* cdf = reinterpret_cast<double*>(S + T_CDF);
    float *va = S + T_VA, *vb = S + T_VB, *vc = S + T_VC, *vm = S + T_VM;
    // the lane predicates as VGPR values: held as 64-bit lane masks across the block loop they crowded the SGPRs that the weight
    // stream double-buffers (spills through v_writelane, weights copied to VGPRs)
    int act_v = set < SZ_SETS ? 1 : 0, live_v = live ? 1 : 0;
    asm volatile("" : "+v"(act_v), "+v"(live_v));
    float* trow = tile + q * ROW;                                    // the lane's own particle row

    const size_t slot = (size_t)own * a_.N + n;
    float h0[H];
    {
        const float4* hp = reinterpret_cast<const float4*>(a_.h + slot * SP * H) + q;
#pragma unroll
        for (int u = 0; u < H; u += 4) {
            const float4 v = hp[(u / 4) * SP];
            h0[u] = v.x; h0[u + 1] = v.y; h0[u + 2] = v.z; h0[u + 3] = v.w;
        }
    }
    float p0 = a_.p[slot * SP + q];
    const float al = a_.alpha, floor_ = a_.floor_;

    for (int s_ = 0; s_ < a_.steps; ++s_) {
        int lim = a_.N;                                              // the sets this step reports for
#pragma unroll
        for (int j = 1; j < SZ_MAXSTEPS; ++j) lim = (j == s_) ? a_.Ns[j - 1] : lim;
        if (s_ > 0 && __builtin_amdgcn_readfirstlane(__syncthreads_or((live_v && n < lim) ? 1 : 0)) == 0) break;   // no set of the workgroup still runs
        const float* wl = a_.w + (size_t)own * L.stride;
        int ql = q, nl = n;
        asm volatile("" : "+s"(wl));                                 // (separate statements: an asm with a VGPR output is divergent)
        asm volatile("" : "+v"(p0), "+v"(ql), "+v"(nl));
        const int qq = ql, nn = nl;
        const rs_cmem_t W = rs_as_cmem(wl);
        float x[SIN];
        {
            const float* o = a_.obs + (size_t)s_ * a_.step_stride * RS_OBS_DIM + ((size_t)nn * a_.A + own) * RS_OBS_DIM;
#pragma unroll
            for (int k = 0; k < SIN; ++k) x[k] = o[k];
        }
        uint64_t k_res = 0, pk = 0;
        if constexpr (!REC) {
            const uint64_t kb = rs_draw_base(a_.base[slot]);
            const uint64_t ctr8 = rs_draw_counter(a_.episode[nn], a_.calls[nn + (size_t)s_ * a_.step_stride]);
            k_res = rs_draw_key(kb, ctr8 + 2ull);
            pk = rs_draw_lane(rs_draw_key(kb, ctr8 + 1ull), qq);
        }
        // h0 into the lane's own tile row: pass 2 reads it back by runtime unit index (the previous step's last tile reads were
        // before its barrier 8)
        if (act_v) {
#pragma unroll
            for (int u = 0; u < H; ++u) trow[u] = h0[u];
        }
        // ---- pass 1: r * h0 (registers), 16 columns of W_r at a time (an 8-wide last chunk when H is 8 mod 16)
        float rh[H];
        auto cv1 = [&](int k) -> float { return (k < H) ? h0[k < H ? k : 0] : x[(k >= H && k < K) ? k - H : 0]; };
        auto rchunk = [&](auto c0, auto nc) {
            constexpr int C0 = decltype(c0)::value, NC = decltype(nc)::value;
            float acc[NC];
#pragma unroll
            for (int o = 0; o < NC; ++o) { acc[o] = W[L.RB + C0 + o]; asm volatile("" : "+v"(acc[o])); }
            rs_ss_mv_cols<K, H, C0, NC>(W + L.R, cv1, acc);
#pragma unroll
            for (int o = 0; o < NC; ++o) rh[C0 + o] = rs_sigmoid(acc[o]) * h0[C0 + o];
        };
        using I16 = std::integral_constant<int, 16>;
        if constexpr (H >= 16) rchunk(std::integral_constant<int, 0>{}, I16{});
        if constexpr (H >= 32) rchunk(std::integral_constant<int, 16>{}, I16{});
        if constexpr (H >= 48) rchunk(std::integral_constant<int, 32>{}, I16{});
        if constexpr (H >= 64) rchunk(std::integral_constant<int, 48>{}, I16{});
        if constexpr (H % 16 == 8) rchunk(std::integral_constant<int, H - 8>{}, std::integral_constant<int, 8>{});
        // ---- pass 2: per 8-unit block (runtime loop) z and the candidate; h1 into the tile row; the observation logit
        auto cv2 = [&](int k) -> float { return (k < H) ? rh[k < H ? k : 0] : x[(k >= H && k < K) ? k - H : 0]; };
        float lg = W[L.OB];
#pragma unroll 1
        for (int b = 0; b < H / 8; ++b) {
            const float* wb = wl + L.ZN + b * (K * 24);
            asm volatile("" : "+s"(wb));                             // per block: nothing of a block is requested before its turn
            // the inputs re-enter every block: otherwise the (c, c) operand pairs of the packed FMAs are hoisted out of the loop,
            // two VGPRs per input and vector (345 VGPRs at 64 units, spilling into AGPRs)
#pragma unroll
            for (int k = 0; k < H; ++k) asm volatile("" : "+v"(h0[k]), "+v"(rh[k]));
            const rs_cmem_t WB = rs_as_cmem(wb);
            const rs_cmem_t BB = W + L.ZNB + b * 24;
            float az[8], an[16];
#pragma unroll
            for (int o = 0; o < 8; ++o) { az[o] = BB[o]; asm volatile("" : "+v"(az[o])); }      // the biases in VGPRs: a v_pk_fma
#pragma unroll                                                                                             // takes one SGPR pair (the weights)
            for (int o = 0; o < 16; ++o) { an[o] = BB[8 + o]; asm volatile("" : "+v"(an[o])); }
            rs_ss_mv_cols<K, 24, 0, 8>(WB, cv1, az);
            rs_ss_mv_cols<K, 24, 8, 16>(WB, cv2, an);
            float eps8[8];
#pragma unroll
            for (int w = 0; w < 8; w += 2) {
                const int u = 8 * b + w;
                if constexpr (REC) {
                    eps8[w] = a_.eps_in[(slot * SP + qq) * H + u];
                    eps8[w + 1] = a_.eps_in[(slot * SP + qq) * H + u + 1];
                } else {
                    rs_hash_normal_pair(rs_hash_bits(pk + (uint64_t)u), eps8[w], eps8[w + 1]);      // one hash per pair of units
                }
            }
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const int u = 8 * b + w;
                const float z = rs_sigmoid(az[w]);
                const float var = an[8 + w];
                const float sp = (var > 20.0f) ? var : 0.69314718f * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(1.44269504f * var));
                const float y = an[w] + eps8[w] * sp;
                const float nv = rs_tanh(y);
                const float h1 = (1.0f - z) * nv + z * trow[u];
                if (act_v) trow[u] = h1;
                lg = fmaf(W[L.O + u], h1, lg);
            }
        }
#pragma unroll
        for (int k = 0; k < SIN; ++k) lg = fmaf(W[L.O + H + k], x[k], lg);
        // ---- observation likelihood, log-softmax over the set's particles (K11 from here on)
        lg += p0;
        if (act_v) va[qq] = lg;
        __syncthreads();                                                // 1
        const float mx = rs_max40(va);
        const float e1 = rs_exp(lg - mx);
        if (act_v) vb[qq] = e1;
        __syncthreads();                                                // 2
        float p1 = (lg - mx) - rs_log(rs_sum40(vb));
        if (act_v) {
            va[qq] = al * rs_exp(p1) + floor_;
            vc[qq] = p1;
        }
        __syncthreads();                                                // 3
        int idx = 0;
        if constexpr (REC) {
            idx = min(max(a_.idx_in[slot * SP + qq], 0), SP - 1);
        } else {
            double mine, run;                                           // float64 prefix sums in index order
            rs_prefix40(va, qq, mine, run);
            if (act_v) cdf[qq] = mine / run;
            __syncthreads();                                            // 4
            idx = min(rs_search40(cdf, rs_hash_uniform(rs_draw_lane(k_res, qq))), SP - 1);      // searchsorted(..., right=True)
        }
        const float* grow = tile + idx * ROW;
#pragma unroll
        for (int u = 0; u < H; ++u) h0[u] = grow[u];                   // the resampled particle: the carried state / next step's input
        float pn = rs_exp(vc[idx]);
        pn = rs_log(pn * __builtin_amdgcn_rcpf(al * pn + floor_));
        if (act_v) vb[qq] = pn;
        __syncthreads();                                                // 5
        const float mx2 = rs_max40(vb);
        const float e2 = rs_exp(pn - mx2);
        if (act_v) va[qq] = e2;
        __syncthreads();                                                // 6
        p1 = pn - (rs_log(rs_sum40(va)) + mx2);
        p0 = p1;
        // ---- weighted mean of the particles, then hid_obs: Linear(H, 24)-ReLU-Linear(24, 2)-ReLU
        const float wgt = rs_exp(p1);
        if (act_v) {
#pragma unroll
            for (int u = 0; u < H; ++u) trow[u] = wgt * h0[u];         // every lane gathered its row before barrier 5
        }
        __syncthreads();                                                // 7
        for (int u = qq; u < H; u += SP) {
            float mean = 0.0f;
            for (int j = 0; j < SP; ++j) mean += tile[j * ROW + u];
            if (act_v) vm[u] = mean;
        }
        __syncthreads();                                                // 8
        const float* wg = wl;
        const int ul = qq < 24 ? qq : 23;
        float t = wg[L.H0B + ul];
        for (int k = 0; k < H; ++k) t = fmaf(wg[L.H0 + k * 24 + ul], vm[k], t);
        t = fmaxf(t, 0.0f);
        if (act_v && qq < 24) { vb[qq] = wg[L.H2 + ul] * t; vc[qq] = wg[L.H2 + 24 + ul] * t; }   // vb / vc: last read before barrier 6
        __syncthreads();                                                // 9
        if (live_v && qq == 0 && nn < lim) {
            float o0 = 0.0f, o1 = 0.0f;
            for (int k = 0; k < 24; ++k) { o0 += vb[k]; o1 += vc[k]; }
            float* out = a_.pred + (size_t)s_ * a_.step_stride * 2 + ((size_t)nn * a_.A + own) * 2;
            out[0] = fmaxf(o0 + wg[L.H2B], 0.0f); out[1] = fmaxf(o1 + wg[L.H2B + 1], 0.0f);
        }
    }
    if (a_.carry && live_v) {
        float4* hw = reinterpret_cast<float4*>(a_.h + slot * SP * H) + q;
#pragma unroll
        for (int u = 0; u < H; u += 4) hw[(u / 4) * SP] = make_float4(h0[u], h0[u + 1], h0[u + 2], h0[u + 3]);
        a_.p[slot * SP + q] = p0;
    }
}

template <bool REC>
int launch(int H, const SzArgs& a, int groups, int A, hipStream_t st) {
    const dim3 g((unsigned)(groups * A)), b(SZ_NT);
    switch (H) {
        case 8: hipLaunchKernelGGL((rs_pfgru_sized_kernel<8, REC>), g, b, 0, st, a, groups); break;
        case 16: hipLaunchKernelGGL((rs_pfgru_sized_kernel<16, REC>), g, b, 0, st, a, groups); break;
        case 24: hipLaunchKernelGGL((rs_pfgru_sized_kernel<24, REC>), g, b, 0, st, a, groups); break;
        case 32: hipLaunchKernelGGL((rs_pfgru_sized_kernel<32, REC>), g, b, 0, st, a, groups); break;
        case 40: hipLaunchKernelGGL((rs_pfgru_sized_kernel<40, REC>), g, b, 0, st, a, groups); break;
        case 48: hipLaunchKernelGGL((rs_pfgru_sized_kernel<48, REC>), g, b, 0, st, a, groups); break;
        case 56: hipLaunchKernelGGL((rs_pfgru_sized_kernel<56, REC>), g, b, 0, st, a, groups); break;
        case 64: hipLaunchKernelGGL((rs_pfgru_sized_kernel<64, REC>), g, b, 0, st, a, groups); break;
        default: return RS_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

SzArgs make_args(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                 const int64_t* calls, const uint8_t* mask, float* pred, const float* eps, const int32_t* idx, int N, int A, int carry,
                 double alpha) {
    SzArgs a{};
    a.w = weights; a.obs = obs; a.h = h; a.p = p; a.base = base_key; a.episode = episode; a.calls = calls; a.mask = mask; a.pred = pred;
    a.eps_in = eps; a.idx_in = idx; a.N = N; a.A = A; a.carry = carry; a.steps = 1; a.step_stride = 0;
    a.alpha = (float)alpha; a.floor_ = (float)((1.0 - alpha) / (double)SP);
    return a;
}

}  // namespace

extern "C" {

int32_t rs_pfgru_sized_weight_floats(int32_t hidden) { return width_ok(hidden) ? (int32_t)slayout(hidden).stride : 0; }

int rs_pfgru_sized_step(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                        const int64_t* calls, const uint8_t* mask, int32_t carry_hidden, double alpha, float* pred, int32_t num_envs,
                        int32_t num_agents, int32_t hidden, rs_stream_t stream) {
    if (!width_ok(hidden)) return RS_ERR_UNSUPPORTED;
    if (!weights || !obs || !h || !p || !base_key || !episode || !calls || !pred || num_envs < 1 || num_agents < 1 || num_agents > RS_MAX_AGENTS)
        return RS_ERR_INVALID_ARG;
    const SzArgs a = make_args(weights, obs, h, p, base_key, episode, calls, mask, pred, nullptr, nullptr, num_envs, num_agents,
                               carry_hidden ? 1 : 0, alpha);
    return launch<false>(hidden, a, (num_envs + SZ_SETS - 1) / SZ_SETS, num_agents, static_cast<hipStream_t>(stream));
}

int rs_pfgru_sized_pass(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                        const int64_t* calls, double alpha, float* pred, const int32_t* alive, int32_t steps, int32_t episodes, int32_t hidden,
                        rs_stream_t stream) {
    if (!width_ok(hidden)) return RS_ERR_UNSUPPORTED;
    if (!weights || !obs || !h || !p || !base_key || !episode || !calls || !pred || !alive || steps < 1 || episodes < 1) return RS_ERR_INVALID_ARG;
    for (int t = 0; t < steps; ++t)
        if (alive[t] < 0 || alive[t] > episodes || (t > 0 && alive[t] > alive[t - 1])) return RS_ERR_INVALID_ARG;
    int rc = rs_pfgru_sized_reset(h, p, base_key, episode, calls, nullptr, episodes, 1, hidden, stream);      // csrc/rs_draws.hip
    // launches of up to PASS_STEPS steps over the episodes alive at their first step; an episode that ends inside a launch's steps
    // reports only its own steps (its extra steps are computed and discarded), a workgroup whose sets have all ended leaves
    constexpr int PASS_STEPS = RS_PFGRU_SIZED_PASS_STEPS;
    for (int t = 0; t < steps && rc == RS_OK && alive[t] > 0;) {
        SzArgs a = make_args(weights, obs + (size_t)t * episodes * RS_OBS_DIM, h, p, base_key, episode, calls + (size_t)t * episodes, nullptr,
                             pred + (size_t)t * episodes * 2, nullptr, nullptr, alive[t], 1, 1, alpha);
        int s_ = 1;
        for (; s_ < PASS_STEPS && t + s_ < steps && alive[t + s_] > 0; ++s_) a.Ns[s_ - 1] = alive[t + s_];
        a.steps = s_;
        a.step_stride = episodes;
        rc = launch<false>(hidden, a, (alive[t] + SZ_SETS - 1) / SZ_SETS, 1, static_cast<hipStream_t>(stream));
        t += s_;
    }
    return rc;
}

int rs_pfgru_sized_step_recorded(const float* weights, const float* obs, float* h, float* p, const float* eps, const int32_t* idx,
                                 const uint8_t* mask, int32_t carry_hidden, double alpha, float* pred, int32_t num_envs, int32_t num_agents,
                                 int32_t hidden, rs_stream_t stream) {
    if (!width_ok(hidden)) return RS_ERR_UNSUPPORTED;
    if (!weights || !obs || !h || !p || !eps || !idx || !pred || num_envs < 1 || num_agents < 1 || num_agents > RS_MAX_AGENTS)
        return RS_ERR_INVALID_ARG;
    const SzArgs a = make_args(weights, obs, h, p, nullptr, nullptr, nullptr, mask, pred, eps, idx, num_envs, num_agents,
                               carry_hidden ? 1 : 0, alpha);
    return launch<true>(hidden, a, (num_envs + SZ_SETS - 1) / SZ_SETS, num_agents, static_cast<hipStream_t>(stream));
}

}  // extern "C"

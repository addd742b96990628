// rs_rnn_sized.hip -- the RAD-A2C actor-critic (GRU + one-hidden-layer policy and value heads) at widths other than the CLI default
// (SURVEY section 8 row f2): the counterparts of K14 (policy step), K12 (GRU time loop + BPTT) and K15 (heads + PPO loss + backward)
// for a GRU of 1..64 units and heads of 2..64 units (main.py --hid-gru / --hid-pol / --hid-val; RADA2C_core.py:484-495
// defaults to 32 / 64 / 64).  The default-size kernels (rs_gru.hip, rs_rnn_policy.hip) are untouched and still serve (24, 32, 32).
//
// Mapping: one env / episode / sample per lane, as K12 - K15.  The GRU width is padded to a compile-time tier HT (16, 32, 48, 64):
// a padded unit has zero weights and zero state, so r = z = 0.5, n = tanh(0) = 0 and it stays exactly 0.  Only the GRU state lives
// in registers (old and new state: 2 HT VGPRs); the gates are formed in blocks of 8 units (r | z | n: 24 columns) so that no
// [3 HT] gate vector is ever held.  The heads are streamed in blocks of 8 hidden units with the logits / value accumulated per
// block: the head width is a runtime loop and only the GRU tier is a template parameter.  A padded head unit has zero weights:
// tanh(0) = 0 into a zero column.  Weights are wave-uniform and stream through the scalar unit (csrc/rs_sstream.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_draws.hpp"
#include "rs_sstream.hpp"

namespace {

constexpr int NX = RS_OBS_DIM + 2, NA = 8;     // 13 GRU inputs, 8 actions

__host__ __device__ constexpr int tier_of(int hid) { return ((hid + 15) / 16) * 16; }

// ---- packed policy weights (floats; packer: radiation_ppo_amd/rada2c.py: pack_sized_policy_weights), for tier HT, nb = HT / 8 unit
// blocks, npb = ceil(pol / 8) policy-head blocks, nvb = ceil(val / 8) value-head blocks:
//   GRU block b (nb of them, GB floats each): IH [13][24] | BIH [24] | HH [HT][24] | BHH [24]
//       column g * 8 + i of a block = gate g (r, z, n) of unit 8 b + i; row k = input / state unit k (k-major W^T)
//   policy block c (npb, PB floats): W1 [HT][8] | B1 [8] | W2 [8 units][8 actions] | W1T [8][HT] | W2T [8 actions][8 units]
//   value block c (nvb, VB floats):  V1 [HT][8] | VB1 [8] | V2 [8] | V1T [8][HT]
//   tail [16]: b2 [8] | vb2 | 0 x 7
__host__ __device__ constexpr int gru_block(int HT) { return 24 * (NX + 1 + HT + 1); }
__host__ __device__ constexpr int pol_block(int HT) { return 16 * HT + 8 + 128; }
__host__ __device__ constexpr int val_block(int HT) { return 16 * HT + 16; }
__host__ __device__ constexpr int nblk8(int w) { return (w + 7) / 8; }
__host__ __device__ constexpr long long policy_floats(int hid, int pol, int val) {
    return (long long)(tier_of(hid) / 8) * gru_block(tier_of(hid)) + (long long)nblk8(pol) * pol_block(tier_of(hid))
           + (long long)nblk8(val) * val_block(tier_of(hid)) + 16;
}
// ---- packed sequence weights (packer: rada2c.py: pack_sized_gru_weights): HH [nb][HT][24] | BHH [nb][24] | HHB [nb][24][HT]
//   (HHB: block b's 24 rows of W_hh (gate g, unit 8 b + i) over its HT columns -- the transposed product of the backward walk)
__host__ __device__ constexpr long long gru_floats(int hid) { return (long long)(tier_of(hid) / 8) * (48 * tier_of(hid) + 24); }

bool widths_ok(int hid, int pol, int val) { return hid >= 1 && hid <= 64 && pol >= 2 && pol <= 64 && val >= 2 && val <= 64; }

// acc[24] += W^T c over a k-major [K][24] block (16 + 8 columns)
template <int K, typename F>
__device__ __forceinline__ void mv24(rs_cmem_t W, F cval, float (&acc)[24]) {
    float a[16], b[8];
#pragma unroll
    for (int o = 0; o < 16; ++o) a[o] = acc[o];
#pragma unroll
    for (int o = 0; o < 8; ++o) b[o] = acc[16 + o];
    rs_ss_mv_cols<K, 24, 0, 16>(W, cval, a);
    rs_ss_mv_cols<K, 24, 16, 8>(W, cval, b);
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = a[o];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[16 + o] = b[o];
}

// 8 consecutive floats of a row at column c0 (c0 a multiple of 8) whose real length is n: entries past n read as 0 / are not written.
// Rows whose length is a multiple of 4 travel as float4 (16-byte aligned when the tensor is), others float by float.
__device__ __forceinline__ void ld8(const float* __restrict__ row, int c0, int n, float (&v)[8]) {
    if ((n & 3) == 0 && c0 + 8 <= n) {
        const float4 p = *reinterpret_cast<const float4*>(row + c0), q = *reinterpret_cast<const float4*>(row + c0 + 4);
        v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = c0 + i < n ? row[c0 + i] : 0.0f;
    }
}
__device__ __forceinline__ void st8(float* __restrict__ row, int c0, int n, const float* v) {
    if ((n & 3) == 0 && c0 + 8 <= n) {
        *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(row + c0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (c0 + i < n) row[c0 + i] = v[i];
    }
}

// h' = GRU(x, h) for a state in registers: block b of 8 units at a time from the packed GRU blocks (IH | BIH | HH | BHH)
template <int HT>
__device__ __forceinline__ void gru_cell(rs_cmem_t W, const float (&x)[NX], const float (&h)[HT], float (&hn)[HT]) {
#pragma unroll
    for (int b = 0; b < HT / 8; ++b) {
        const rs_cmem_t Wb = W + b * gru_block(HT);
        float gi[24], gh[24];
#pragma unroll
        for (int o = 0; o < 24; ++o) { gi[o] = Wb[NX * 24 + o]; gh[o] = Wb[(NX + 1 + HT) * 24 + o]; }
        mv24<NX>(Wb, [&](int k) -> float { return x[k]; }, gi);
        mv24<HT>(Wb + (NX + 1) * 24, [&](int k) -> float { return h[k]; }, gh);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float r = rs_sigmoid(gi[i] + gh[i]);
            const float z = rs_sigmoid(gi[8 + i] + gh[8 + i]);
            const float n = rs_tanh(gi[16 + i] + r * gh[16 + i]);
            hn[8 * b + i] = (1.0f - z) * n + z * h[8 * b + i];
        }
    }
}

// logits (8) and value of both heads for a state in registers; head blocks streamed (runtime loop over 8-unit blocks)
template <int HT>
__device__ __forceinline__ void heads_fwd(const float* w, int pol_at, int npb, int val_at, int nvb, int tail_at, const float (&h)[HT],
                                          float (&lg)[8], float& value, bool want_pol, bool want_val) {
    const rs_cmem_t W = rs_as_cmem(w);
#pragma unroll
    for (int o = 0; o < 8; ++o) lg[o] = W[tail_at + o];
    value = W[tail_at + 8];
    if (want_pol) {
        for (int c = 0; c < npb; ++c) {
            const float* wp = w + pol_at + c * pol_block(HT); asm volatile("" : "+s"(wp));
            const rs_cmem_t P = rs_as_cmem(wp);
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = P[8 * HT + i];
            rs_ss_mv_cols<HT, 8, 0, 8>(P, [&](int k) -> float { return h[k]; }, t);
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = rs_tanh(t[i]);
            rs_ss_mv_cols<8, 8, 0, 8>(P + 8 * HT + 8, [&](int k) -> float { return t[k]; }, lg);
        }
    }
    if (want_val) {
        float v0 = value, v1 = 0.0f;
        for (int c = 0; c < nvb; ++c) {
            const float* wp = w + val_at + c * val_block(HT); asm volatile("" : "+s"(wp));
            const rs_cmem_t V = rs_as_cmem(wp);
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = V[8 * HT + i];
            rs_ss_mv_cols<HT, 8, 0, 8>(V, [&](int k) -> float { return h[k]; }, t);
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                v0 = fmaf(V[8 * HT + 8 + i], rs_tanh(t[i]), v0);
                v1 = fmaf(V[8 * HT + 8 + i + 1], rs_tanh(t[i + 1]), v1);
            }
        }
        value = v0 + v1;
    }
}

struct Layout {
    int pol_at, npb, val_at, nvb, tail_at;
};
template <int HT>
Layout layout(int pol, int val) {
    Layout l;
    l.pol_at = (HT / 8) * gru_block(HT);
    l.npb = nblk8(pol);
    l.val_at = l.pol_at + l.npb * pol_block(HT);
    l.nvb = nblk8(val);
    l.tail_at = l.val_at + l.nvb * val_block(HT);
    return l;
}

struct StepArgs {
    const float* w;
    const float* x; const float* loc; const float* h; const float* u;
    float* h_out; float* logits; float* value; int64_t* act; float* logp;
    int8_t* act8;
    const uint8_t* mask;
    int N, hid, xs, ls, us, as;
    Layout l;
};

// the sized policy step (K14's contract): GRU cell, both heads, log-softmax, inverse-CDF draw on the caller's uniform
// The draw of this kernel and of the team kernel below is csrc/rs_action.hpp's text written out (keep them in step by hand): on the
// shared copy the sized per-agent bootstrap round at 4096 envs timed 0.0658 ms against 0.0657 ms + 0.0001 ms of spread and a sized
// team epoch with eight agents 214.98 ms against 214.62 ms + 0.29 ms (three alternated rounds each; every five-round row was inside
// its spread), outside the rule (profiles/policy_pieces_timing.txt).
template <int HT>
__global__ void __launch_bounds__(64) rs_rnn_sized_step_kernel(StepArgs a_) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    const bool live = e < a_.N && (a_.mask == nullptr || a_.mask[e] != 0);
    if (!__any(live)) return;
    const int ec = e < a_.N ? e : a_.N - 1;                // idle lanes shadow a real env, store nothing
    float x[NX], h[HT], hn[HT];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) x[k] = a_.x[(size_t)ec * a_.xs + k];
    x[RS_OBS_DIM] = a_.loc[(size_t)ec * a_.ls]; x[RS_OBS_DIM + 1] = a_.loc[(size_t)ec * a_.ls + 1];
    const float* hrow = a_.h + (size_t)ec * a_.hid;
#pragma unroll
    for (int b = 0; b < HT / 8; ++b) {
        float v[8];
        ld8(hrow, 8 * b, a_.hid, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) h[8 * b + i] = v[i];
    }
    gru_cell<HT>(rs_as_cmem(a_.w), x, h, hn);
    if (a_.h_out && live) {
        float* orow = a_.h_out + (size_t)e * a_.hid;
#pragma unroll
        for (int b = 0; b < HT / 8; ++b) st8(orow, 8 * b, a_.hid, hn + 8 * b);
    }
    const bool want_pol = a_.logits || a_.act || a_.logp || a_.act8;
    float lg[8], val;
    heads_fwd<HT>(a_.w, a_.l.pol_at, a_.l.npb, a_.l.val_at, a_.l.nvb, a_.l.tail_at, hn, lg, val, want_pol, a_.value != nullptr);
    if (a_.value && live) a_.value[e] = val;
    if (a_.logits && live) {
        *reinterpret_cast<float4*>(a_.logits + (size_t)e * NA) = make_float4(lg[0], lg[1], lg[2], lg[3]);
        *reinterpret_cast<float4*>(a_.logits + (size_t)e * NA + 4) = make_float4(lg[4], lg[5], lg[6], lg[7]);
    }
    if (a_.act || a_.logp || a_.act8) {
        float mx = lg[0];
#pragma unroll
        for (int o = 1; o < NA; ++o) mx = fmaxf(mx, lg[o]);
        float se = 0.0f;
#pragma unroll
        for (int o = 0; o < NA; ++o) se += expf(lg[o] - mx);
        const float lse = logf(se);
        const float uu = a_.u ? a_.u[(size_t)ec * a_.us] : 0.0f;
        float cdf = 0.0f, lp_sel = (lg[0] - mx) - lse;
        int act = 0;
#pragma unroll
        for (int o = 0; o < NA; ++o) {
            const float lp = (lg[o] - mx) - lse;
            cdf += expf(lp);
            if (o < NA - 1 && cdf <= uu) { act = o + 1; }
        }
#pragma unroll
        for (int o = 1; o < NA; ++o) if (act == o) lp_sel = (lg[o] - mx) - lse;
        if (live) {
            if (a_.act) a_.act[e] = act;
            if (a_.act8) a_.act8[(size_t)e * a_.as] = (int8_t)act;
            if (a_.logp) a_.logp[e] = lp_sel;
        }
    }
}

// the policy round of a whole team in one launch (rs_rnn_team_step's contract, csrc/rs_rnn_policy.hip): grid = (64-lane groups,
// agent), blockIdx.y's agent on its rows of x [N][A][11], loc [N][A][2], u [N][A], act8 [N][A], with its own weights and its own slab
// of h [A][N][hid], updated in place (a lane has its row in registers before it stores).  u given: the step round -- h, the action
// (act [A][N], act8) and, when f = logp_val_boot [A][3][N] is given, the log-probability (slot 0) and the value (slot 1); u null: the
// bootstrap round -- the value of the GRU's next state (slot 2) and nothing else.  The pieces are rs_rnn_sized_step_kernel's.
struct TeamStepArgs {
    const float* w[RS_MAX_AGENTS];   // the weight pointers travel in the argument block
    const float* x; const float* loc; float* h; const float* u;
    int64_t* act; float* f; int8_t* act8;
    const uint8_t* mask;
    int N, A, hid;
    Layout l;
};

template <int HT>
__global__ void __launch_bounds__(64) rs_rnn_sized_team_kernel(TeamStepArgs t) {
    const int e = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y;
    const bool live = e < t.N && (t.mask == nullptr || t.mask[e] != 0);
    if (!__any(live)) return;
    const int ec = e < t.N ? e : t.N - 1;                  // idle lanes shadow a real env, store nothing
    const float* w = t.w[a];
    const size_t i = (size_t)ec * t.A + a;
    const bool step = t.u != nullptr;
    float x[NX], h[HT], hn[HT];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) x[k] = t.x[i * RS_OBS_DIM + k];
    x[RS_OBS_DIM] = t.loc[i * 2]; x[RS_OBS_DIM + 1] = t.loc[i * 2 + 1];
    float* hrow = t.h + ((size_t)a * t.N + ec) * t.hid;
#pragma unroll
    for (int b = 0; b < HT / 8; ++b) {
        float v[8];
        ld8(hrow, 8 * b, t.hid, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) h[8 * b + k] = v[k];
    }
    gru_cell<HT>(rs_as_cmem(w), x, h, hn);
    if (step && live) {
#pragma unroll
        for (int b = 0; b < HT / 8; ++b) st8(hrow, 8 * b, t.hid, hn + 8 * b);
    }
    float lg[8], val;
    heads_fwd<HT>(w, t.l.pol_at, t.l.npb, t.l.val_at, t.l.nvb, t.l.tail_at, hn, lg, val, step, t.f != nullptr);
    float* frow = t.f ? t.f + (size_t)a * 3 * t.N + ec : nullptr;          // slot s of this lane: frow[s N]
    if (frow && live) frow[(size_t)(step ? 1 : 2) * t.N] = val;
    if (!step) return;
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NA; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NA; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
    const float uu = t.u[i];
    float cdf = 0.0f, lp_sel = (lg[0] - mx) - lse;
    int act = 0;
#pragma unroll
    for (int o = 0; o < NA; ++o) {
        const float lp = (lg[o] - mx) - lse;
        cdf += expf(lp);
        if (o < NA - 1 && cdf <= uu) { act = o + 1; }
    }
#pragma unroll
    for (int o = 1; o < NA; ++o) if (act == o) lp_sel = (lg[o] - mx) - lse;
    if (live) {
        if (t.act) t.act[(size_t)a * t.N + e] = act;
        if (t.act8) t.act8[i] = (int8_t)act;
        if (frow) *frow = lp_sel;
    }
}

// ---- GRU sequence (K12's contract at any width): gi [L][E][3 hid], h0 [E][hid] -> hs [L][E][hid], gates [L][E][4 HT]
//      (per 8-unit block: r | z | n | W_hn h + b_hn, 32 floats)
template <int HT>
__global__ void __launch_bounds__(64) rs_gru_sized_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ h0, const float* __restrict__ wg,
                                                              float* __restrict__ hs, float* __restrict__ gates, int hid, int L, int E) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    const int ec = e < E ? e : E - 1;
    const int G = 3 * hid;
    float h[HT];
#pragma unroll
    for (int b = 0; b < HT / 8; ++b) {
        float v[8];
        ld8(h0 + (size_t)ec * hid, 8 * b, hid, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) h[8 * b + i] = v[i];
    }
    for (int t = 0; t < L; ++t) {
        const float* wp = wg; asm volatile("" : "+s"(wp));                      // per step: keeps LICM from hoisting the rows
        const rs_cmem_t W = rs_as_cmem(wp);
        const size_t te = (size_t)t * E + ec;
        const float* girow = gi + te * G;
        float hn[HT];
#pragma unroll
        for (int b = 0; b < HT / 8; ++b) {
            float g[24], gh[24];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float v[8];
                ld8(girow + q * hid, 8 * b, hid, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) g[8 * q + i] = v[i];
            }
            const rs_cmem_t B = W + (HT / 8) * HT * 24 + b * 24;
#pragma unroll
            for (int o = 0; o < 24; ++o) gh[o] = B[o];
            mv24<HT>(W + b * HT * 24, [&](int k) -> float { return h[k]; }, gh);
            float go[32];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float r = rs_sigmoid(g[i] + gh[i]);
                const float z = rs_sigmoid(g[8 + i] + gh[8 + i]);
                const float hh = gh[16 + i];
                const float n = rs_tanh(g[16 + i] + r * hh);
                hn[8 * b + i] = (1.0f - z) * n + z * h[8 * b + i];
                go[i] = r; go[8 + i] = z; go[16 + i] = n; go[24 + i] = hh;
            }
            if (e < E) {
                float* gp = gates + te * (4 * HT) + 32 * b;
#pragma unroll
                for (int u = 0; u < 32; u += 4) *reinterpret_cast<float4*>(gp + u) = make_float4(go[u], go[u + 1], go[u + 2], go[u + 3]);
            }
        }
        if (e < E) {
#pragma unroll
            for (int b = 0; b < HT / 8; ++b) st8(hs + te * hid, 8 * b, hid, hn + 8 * b);
        }
#pragma unroll
        for (int j = 0; j < HT; ++j) h[j] = hn[j];
    }
}

// backward: dhs [L][E][hid], hs, gates, h0 -> dgi [L][E][3 hid] = dL/d(gi), dgh [L][E][3 hid] = dL/d(W_hh h + b_hh)
template <int HT>
__global__ void __launch_bounds__(64) rs_gru_sized_bwd_kernel(const float* __restrict__ dhs, const float* __restrict__ hs, const float* __restrict__ gates,
                                                              const float* __restrict__ h0, const float* __restrict__ wg, float* __restrict__ dgi,
                                                              float* __restrict__ dgh, int hid, int L, int E) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    const int ec = e < E ? e : E - 1;
    const int G = 3 * hid;
    float dh[HT];
#pragma unroll
    for (int j = 0; j < HT; ++j) dh[j] = 0.0f;
    for (int t = L - 1; t >= 0; --t) {
        const float* wp = wg; asm volatile("" : "+s"(wp));
        const rs_cmem_t WB = rs_as_cmem(wp) + (HT / 8) * (HT * 24 + 24);
        const size_t te = (size_t)t * E + ec;
        const float* hprow = t > 0 ? hs + (te - E) * hid : h0 + (size_t)ec * hid;
        float nxt[HT];                                    // dL/dh_{t-1}: d * z (direct path) + W_hh^T dgh, block by block
#pragma unroll
        for (int j = 0; j < HT; ++j) nxt[j] = 0.0f;
#pragma unroll
        for (int b = 0; b < HT / 8; ++b) {
            float dx[8], hp[8], go[32];
            ld8(dhs + te * hid, 8 * b, hid, dx);
            ld8(hprow, 8 * b, hid, hp);
            const float* gp = gates + te * (4 * HT) + 32 * b;
#pragma unroll
            for (int u = 0; u < 32; u += 4) {
                const float4 v = *reinterpret_cast<const float4*>(gp + u);
                go[u] = v.x; go[u + 1] = v.y; go[u + 2] = v.z; go[u + 3] = v.w;
            }
            float dg[24], di[24];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float d = dh[8 * b + i] + dx[i];
                const float r = go[i], z = go[8 + i], n = go[16 + i], hn = go[24 + i];
                const float dn = d * (1.0f - z) * (1.0f - n * n);
                const float dz = d * (hp[i] - n) * z * (1.0f - z);
                const float dr = dn * hn * r * (1.0f - r);
                dg[i] = dr; dg[8 + i] = dz; dg[16 + i] = dn * r;
                di[i] = dr; di[8 + i] = dz; di[16 + i] = dn;
                nxt[8 * b + i] += d * z;
            }
            if (e < E) {
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    st8(dgi + te * G + g * hid, 8 * b, hid, di + 8 * g);
                    st8(dgh + te * G + g * hid, 8 * b, hid, dg + 8 * g);
                }
            }
            rs_ss_mv<24, HT>(WB + b * 24 * HT, [&](int k) -> float { return dg[k]; }, nxt);
        }
#pragma unroll
        for (int j = 0; j < HT; ++j) dh[j] = nxt[j];
    }
}

}  // namespace
namespace {

// ---- heads-loss (K15's contract at any width): one (step, episode) sample per lane.  Writes dL/dh, the per-sample factors of the
// head weight gradients and per-wave statistics; no atomics, so every run writes the same bits.
//   dfac [S][FD], FD = P8 + V8 + 16: d pre-tanh policy [P8] | d pre-tanh value [V8] | d logits [8] | d value | 0 x 7
//   tfac [S][FT], FT = P8 + V8:      tanh policy [P8] | tanh value [V8]          (P8 / V8: the head widths rounded up to 8)
struct HeadArgs {
    const float* w;
    const float* hs; const int64_t* act; const float* adv; const float* ret; const float* lpo; const float* wt;
    float* dhs; float* dfac; float* tfac; float* stats;
    long long S;
    int hid;
    float clip, vf_coef;
    Layout l;
};

template <int HT>
__device__ __forceinline__ void head_block_fwd(rs_cmem_t P, const float (&h)[HT], float (&t)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = P[8 * HT + i];
    rs_ss_mv_cols<HT, 8, 0, 8>(P, [&](int k) -> float { return h[k]; }, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = rs_tanh(t[i]);
}

template <int HT>
__global__ void __launch_bounds__(64) rs_a2c_sized_heads_kernel(HeadArgs a_) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < a_.S;
    const long long ic = live ? i : a_.S - 1;
    const int P8 = 8 * a_.l.npb, V8 = 8 * a_.l.nvb, FT = P8 + V8, FD = FT + 16;
    const rs_cmem_t W = rs_as_cmem(a_.w);
    float h[HT];
#pragma unroll
    for (int b = 0; b < HT / 8; ++b) {
        float v[8];
        ld8(a_.hs + ic * a_.hid, 8 * b, a_.hid, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) h[8 * b + k] = v[k];
    }
    const float wi = live ? a_.wt[ic] : 0.0f;
    const int a = (int)a_.act[ic];
    const float adv = a_.adv[ic], ret = a_.ret[ic], lpo = a_.lpo[ic];
    float lg[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) lg[o] = W[a_.l.tail_at + o];
    float v0 = W[a_.l.tail_at + 8], v1 = 0.0f;
    for (int c = 0; c < a_.l.npb; ++c) {
        const float* wp = a_.w + a_.l.pol_at + c * pol_block(HT); asm volatile("" : "+s"(wp));
        const rs_cmem_t P = rs_as_cmem(wp);
        float t[8];
        head_block_fwd<HT>(P, h, t);
        rs_ss_mv_cols<8, 8, 0, 8>(P + 8 * HT + 8, [&](int k) -> float { return t[k]; }, lg);
        if (live) st8(a_.tfac + i * FT, 8 * c, FT, t);
    }
    for (int c = 0; c < a_.l.nvb; ++c) {
        const float* wp = a_.w + a_.l.val_at + c * val_block(HT); asm volatile("" : "+s"(wp));
        const rs_cmem_t V = rs_as_cmem(wp);
        float t[8];
        head_block_fwd<HT>(V, h, t);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            v0 = fmaf(V[8 * HT + 8 + k], t[k], v0);
            v1 = fmaf(V[8 * HT + 8 + k + 1], t[k + 1], v1);
        }
        if (live) st8(a_.tfac + i * FT, P8 + 8 * c, FT, t);
    }
    const float val = v0 + v1;
    // ---- per-sample loss terms and derivative (K15's formulas)
    float mx = lg[0];
#pragma unroll
    for (int j = 1; j < NA; ++j) mx = fmaxf(mx, lg[j]);
    float se = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; ++j) se += expf(lg[j] - mx);
    const float lse = logf(se);
    float pj[NA], ent = 0.0f, logp = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const float lp = (lg[j] - mx) - lse;
        pj[j] = expf(lp);
        ent -= pj[j] * lp;
        logp = (a == j) ? lp : logp;
    }
    const float ratio = expf(logp - lpo);
    const float lo = 1.0f - a_.clip, hi = 1.0f + a_.clip;
    const float s1 = ratio * adv, s2 = fminf(fmaxf(ratio, lo), hi) * adv;
    const bool inside = ratio >= lo && ratio <= hi;
    const float g_lp = -wi * (((inside || s1 < s2) ? adv : 0.0f) * ratio);
    float dl[8];
#pragma unroll
    for (int j = 0; j < NA; ++j) dl[j] = g_lp * (((a == j) ? 1.0f : 0.0f) - pj[j]);
    const float diff = val - ret;
    const float dval = 2.0f * a_.vf_coef * wi * diff;
    // ---- back through the heads, block by block (the tanh outputs are recomputed: the same code, the same bits)
    float dh[HT];
#pragma unroll
    for (int j = 0; j < HT; ++j) dh[j] = 0.0f;
    for (int c = 0; c < a_.l.npb; ++c) {
        const float* wp = a_.w + a_.l.pol_at + c * pol_block(HT); asm volatile("" : "+s"(wp));
        const rs_cmem_t P = rs_as_cmem(wp);
        float t[8], dp[8];
        head_block_fwd<HT>(P, h, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) dp[k] = 0.0f;
        rs_ss_mv_cols<8, 8, 0, 8>(P + 16 * HT + 72, [&](int o) -> float { return dl[o]; }, dp);        // W2 dl (W2T block)
#pragma unroll
        for (int k = 0; k < 8; ++k) dp[k] = dp[k] * (1.0f - t[k] * t[k]);
        rs_ss_mv<8, HT>(P + 8 * HT + 72, [&](int k) -> float { return dp[k]; }, dh);                  // + W1^T dp (W1T block)
        if (live) st8(a_.dfac + i * FD, 8 * c, FD, dp);
    }
    for (int c = 0; c < a_.l.nvb; ++c) {
        const float* wp = a_.w + a_.l.val_at + c * val_block(HT); asm volatile("" : "+s"(wp));
        const rs_cmem_t V = rs_as_cmem(wp);
        float t[8], dv[8];
        head_block_fwd<HT>(V, h, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) dv[k] = V[8 * HT + 8 + k] * dval * (1.0f - t[k] * t[k]);
        rs_ss_mv<8, HT>(V + 8 * HT + 16, [&](int k) -> float { return dv[k]; }, dh);
        if (live) st8(a_.dfac + i * FD, P8 + 8 * c, FD, dv);
    }
    if (live) {
#pragma unroll
        for (int b = 0; b < HT / 8; ++b) st8(a_.dhs + i * a_.hid, 8 * b, a_.hid, dh + 8 * b);
        const float tail[8] = {dval, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        st8(a_.dfac + i * FD, FT, FD, dl);
        st8(a_.dfac + i * FD, FT + 8, FD, tail);
    }
    // ---- statistics: weighted sums over the wave
    float st[6] = {wi * (lpo - logp), wi * ent, wi * ((ratio > hi || ratio < lo) ? 1.0f : 0.0f), wi * diff * diff, wi * fminf(s1, s2), wi};
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) st[q] += __shfl_xor(st[q], sft);
    }
    if (threadIdx.x == 0) {
        float* so = a_.stats + (long long)blockIdx.x * 8;
#pragma unroll
        for (int q = 0; q < 6; ++q) so[q] = st[q];
        so[6] = 0.0f; so[7] = 0.0f;
    }
}

}  // namespace

#define RS_TIER_SWITCH(hid, KERNEL, GRID, BLOCK, ...)                                                                              \
    switch (tier_of(hid)) {                                                                                                        \
        case 16: hipLaunchKernelGGL(KERNEL<16>, GRID, BLOCK, 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break;           \
        case 32: hipLaunchKernelGGL(KERNEL<32>, GRID, BLOCK, 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break;           \
        case 48: hipLaunchKernelGGL(KERNEL<48>, GRID, BLOCK, 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break;           \
        default: hipLaunchKernelGGL(KERNEL<64>, GRID, BLOCK, 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break;           \
    }

static Layout layout_rt(int hid, int pol, int val) {
    switch (tier_of(hid)) {
        case 16: return layout<16>(pol, val);
        case 32: return layout<32>(pol, val);
        case 48: return layout<48>(pol, val);
        default: return layout<64>(pol, val);
    }
}

extern "C" {

int32_t rs_rnn_sized_weight_floats(int32_t hid, int32_t pol, int32_t val) {
    return widths_ok(hid, pol, val) ? (int32_t)policy_floats(hid, pol, val) : 0;
}

int32_t rs_gru_sized_weight_floats(int32_t hid) { return hid >= 1 && hid <= 64 ? (int32_t)gru_floats(hid) : 0; }

int32_t rs_gru_sized_gate_floats(int32_t hid) { return hid >= 1 && hid <= 64 ? 4 * tier_of(hid) : 0; }

int rs_rnn_sized_step(const float* weights, int32_t hid, int32_t pol, int32_t val, const float* x, int32_t x_stride, const float* loc,
                      int32_t loc_stride, const float* h, const float* u, int32_t u_stride, float* h_out, float* logits, float* value,
                      int64_t* act, float* logp, int8_t* act8, int32_t act8_stride, const uint8_t* mask, int32_t num_envs, rs_stream_t stream) {
    if (!widths_ok(hid, pol, val)) return RS_ERR_UNSUPPORTED;
    if (!weights || !x || !loc || !h || num_envs < 1 || x_stride < RS_OBS_DIM || loc_stride < 2 || u_stride < 1 || act8_stride < 1)
        return RS_ERR_INVALID_ARG;
    if ((act || logp || act8) && !u) return RS_ERR_INVALID_ARG;
    StepArgs a{weights, x, loc, h, u, h_out, logits, value, act, logp, act8, mask, num_envs, hid, x_stride, loc_stride, u_stride, act8_stride,
               layout_rt(hid, pol, val)};
    RS_TIER_SWITCH(hid, rs_rnn_sized_step_kernel, dim3((num_envs + 63) / 64), dim3(64), a);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_rnn_sized_team_step(const float* const* weights, int32_t num_agents, int32_t hid, int32_t pol, int32_t val, const float* x,
                           const float* loc, float* h, const float* u, int64_t* act, float* logp_val_boot, int8_t* act8, const uint8_t* mask,
                           int32_t num_envs, rs_stream_t stream) {
    if (!widths_ok(hid, pol, val)) return RS_ERR_UNSUPPORTED;
    if (!weights || !x || !loc || !h || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_envs < 1) return RS_ERR_INVALID_ARG;
    if (u ? (!act && !act8) : !logp_val_boot) return RS_ERR_INVALID_ARG;       // a step round draws an action, a bootstrap round a value
    TeamStepArgs t{};
    for (int a = 0; a < RS_MAX_AGENTS; ++a) {
        if (a < num_agents && !weights[a]) return RS_ERR_INVALID_ARG;
        t.w[a] = weights[a < num_agents ? a : 0];                  // the slots behind the team repeat agent 0 (never read)
    }
    t.x = x; t.loc = loc; t.h = h; t.u = u; t.act = act; t.f = logp_val_boot; t.act8 = act8; t.mask = mask;
    t.N = num_envs; t.A = num_agents; t.hid = hid; t.l = layout_rt(hid, pol, val);
    RS_TIER_SWITCH(hid, rs_rnn_sized_team_kernel, dim3((num_envs + 63) / 64, num_agents), dim3(64), t);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_gru_sized_forward(const float* gi, const float* h0, const float* weights, float* hs, float* gates, int32_t hid, int32_t steps,
                         int32_t episodes, rs_stream_t stream) {
    if (hid < 1 || hid > 64) return RS_ERR_UNSUPPORTED;
    if (!gi || !h0 || !weights || !hs || !gates || steps < 1 || episodes < 1) return RS_ERR_INVALID_ARG;
    RS_TIER_SWITCH(hid, rs_gru_sized_fwd_kernel, dim3((episodes + 63) / 64), dim3(64), gi, h0, weights, hs, gates, hid, steps, episodes);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_gru_sized_backward(const float* dhs, const float* hs, const float* gates, const float* h0, const float* weights, float* dgi, float* dgh,
                          int32_t hid, int32_t steps, int32_t episodes, rs_stream_t stream) {
    if (hid < 1 || hid > 64) return RS_ERR_UNSUPPORTED;
    if (!dhs || !hs || !gates || !h0 || !weights || !dgi || !dgh || steps < 1 || episodes < 1) return RS_ERR_INVALID_ARG;
    RS_TIER_SWITCH(hid, rs_gru_sized_bwd_kernel, dim3((episodes + 63) / 64), dim3(64), dhs, hs, gates, h0, weights, dgi, dgh, hid, steps,
                   episodes);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_a2c_sized_heads_loss(const float* weights, int32_t hid, int32_t pol, int32_t val, const float* hs, const int64_t* act, const float* adv,
                            const float* ret, const float* logp_old, const float* sample_weight, float* dhs, float* dfac, float* tfac,
                            float* stats, int64_t samples, double clip_ratio, double vf_coef, rs_stream_t stream) {
    if (!widths_ok(hid, pol, val)) return RS_ERR_UNSUPPORTED;
    if (!weights || !hs || !act || !adv || !ret || !logp_old || !sample_weight || !dhs || !dfac || !tfac || !stats || samples < 1)
        return RS_ERR_INVALID_ARG;
    HeadArgs a{weights, hs, act, adv, ret, logp_old, sample_weight, dhs, dfac, tfac, stats, (long long)samples, hid, (float)clip_ratio,
               (float)vf_coef, layout_rt(hid, pol, val)};
    RS_TIER_SWITCH(hid, rs_a2c_sized_heads_kernel, dim3((unsigned)((samples + 63) / 64)), dim3(64), a);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

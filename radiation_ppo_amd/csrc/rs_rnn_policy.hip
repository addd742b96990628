// rs_rnn_policy.hip -- K14: one step of the RAD-A2C actor-critic behind the PFGRU for every env.
//
// Replaces the part of RNNModelActorCritic.step after the location prediction (NeuralNetworkCores/RADA2C_core.py:528-548):
// hidden = GRU(cat(obs, loc_pred), hidden) (SeqPt.forward :377-381, torch.nn.GRU(13, 24, 1), gate order r, z, n), the policy
// head Woms (Linear-Tanh-Linear, :363-366) with Categorical(logits).sample() / log_prob (:541-544) and the value head Valms
// (:367-368) -- ~35 small library kernels per call in the torch composition, two calls per lock-step of the collector
// (the action and the bootstrap value, algos/multiagent/train.py:334-341, :462-487).
//
// Mapping: one env per lane; the six small products (13 -> 72, 24 -> 72, 24 -> 32 twice, 32 -> 8, 32 -> 1) with wave-uniform
// weights through the scalar unit, as K11 - K13.  The action is drawn by inverse CDF on the uniform the caller supplies (the
// env's Philox stream, as the MLP collectors: documented RNG deviation).  Latency bound: N / 64 waves of ~4 500 FMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_draws.hpp"
#include "rs_handle.hpp"
#include "rs_sstream.hpp"

namespace {

constexpr int GH = RS_GRU_HIDDEN, NX = RS_OBS_DIM + 2, NA = 8, HD = 32;    // 24, 13, 8 actions, 32 head units
// packed weights (floats; packer: radiation_ppo_amd/rada2c.py: pack_policy_weights), every block k-major
constexpr int P_IH = 0;                      // [13][80]  W_ih^T (columns 72..79 zero)
constexpr int P_BIH = P_IH + NX * 80;        // [80]
constexpr int P_HH = P_BIH + 80;             // [24][80]  W_hh^T
constexpr int P_BHH = P_HH + GH * 80;        // [80]
constexpr int P_W1 = P_BHH + 80;             // [24][32]  Woms[0]^T
constexpr int P_B1 = P_W1 + GH * HD;         // [32]
constexpr int P_V1 = P_B1 + HD;              // [24][32]  Valms[0]^T
constexpr int P_VB1 = P_V1 + GH * HD;        // [32]
constexpr int P_W2 = P_VB1 + HD;             // [32][16]  Woms[2]^T (columns 8..15 zero)
constexpr int P_B2 = P_W2 + HD * 16;         // [16]
constexpr int P_V2 = P_B2 + 16;              // [32] Valms[2] weight, [1] bias, pad to 48
constexpr int P_STRIDE = P_V2 + 48;
static_assert(P_STRIDE == RS_RNN_POLICY_WEIGHT_FLOATS, "include/radsearch.h: RS_RNN_POLICY_WEIGHT_FLOATS");

typedef const float __attribute__((address_space(4))) * cmem_t;
__device__ __forceinline__ cmem_t as_cmem(const float* p) { return (cmem_t)(uintptr_t)p; }

// out[OUTP] += W^T c through the scalar-unit weight stream (csrc/rs_sstream.hpp: wait -> request -> FMA blocks of two rows)
template <int K, int OUTP, int OUTR = OUTP, typename F>
__device__ __forceinline__ void mv(cmem_t W, F cval, float (&out)[OUTP]) { rs_ss_mv<K, OUTP, OUTR>(W, cval, out); }

struct PolArgs {
    const float* w;        // [RS_RNN_POLICY_WEIGHT_FLOATS]
    const float* x;        // [N][11] standardised observation
    const float* loc;      // [N][2]  PFGRU location prediction
    const float* h;        // [N][24] GRU state
    const float* u;        // [N] uniforms in [0, 1) or null (no action wanted)
    float* h_out;          // [N][24] or null (may alias h)
    float* logits;         // [N][8] or null
    float* value;          // [N] or null
    int64_t* act;          // [N] or null
    float* logp;           // [N] or null
    int N;
    int xs, ls, us;        // row strides (floats) of x, loc, u: 11 / 2 / 1 for packed rows, A times that for agent a's rows of [N][A][.]
    int8_t* act8;          // [N][as] or null: the action once more as the env's int8 (rs_step's input row)
    int as;
    const uint8_t* mask;   // [N] or null: only these envs are wanted (the bootstrap round); a wave without one leaves at once
};

__global__ void __launch_bounds__(64) rs_rnn_policy_kernel(PolArgs a_) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    const bool live = e < a_.N && (a_.mask == nullptr || a_.mask[e] != 0);
    if (!__any(live)) return;
    const int ec = e < a_.N ? e : a_.N - 1;                // idle lanes shadow a real env, store nothing
    const cmem_t W = as_cmem(a_.w);
    float x[NX], h[GH];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) x[k] = a_.x[(size_t)ec * a_.xs + k];
    x[RS_OBS_DIM] = a_.loc[(size_t)ec * a_.ls]; x[RS_OBS_DIM + 1] = a_.loc[(size_t)ec * a_.ls + 1];
#pragma unroll
    for (int u = 0; u < GH; u += 4) {
        const float4 v = *reinterpret_cast<const float4*>(a_.h + (size_t)ec * GH + u);
        h[u] = v.x; h[u + 1] = v.y; h[u + 2] = v.z; h[u + 3] = v.w;
    }
    float gi[80], gh[80];
#pragma unroll
    for (int o = 0; o < 80; ++o) { gi[o] = W[P_BIH + o]; gh[o] = W[P_BHH + o]; }
    mv<NX, 80, 72>(W + P_IH, [&](int k) -> float { return x[k]; }, gi);             // 72 of the 80 columns are real
    mv<GH, 80, 72>(W + P_HH, [&](int k) -> float { return h[k]; }, gh);
#pragma unroll
    for (int j = 0; j < GH; ++j) {
        const float r = rs_sigmoid(gi[j] + gh[j]);
        const float z = rs_sigmoid(gi[GH + j] + gh[GH + j]);
        const float n = rs_tanh(gi[2 * GH + j] + r * gh[2 * GH + j]);
        h[j] = (1.0f - z) * n + z * h[j];
    }
    if (a_.h_out && live) {
#pragma unroll
        for (int u = 0; u < GH; u += 4) *reinterpret_cast<float4*>(a_.h_out + (size_t)e * GH + u) = make_float4(h[u], h[u + 1], h[u + 2], h[u + 3]);
    }
    // ---- value head
    if (a_.value) {
        float t[HD];
#pragma unroll
        for (int o = 0; o < HD; ++o) t[o] = W[P_VB1 + o];
        mv<GH, HD>(W + P_V1, [&](int k) -> float { return h[k]; }, t);
        float v0 = W[P_V2 + HD], v1 = 0.0f;
#pragma unroll
        for (int k = 0; k < HD; k += 2) {
            v0 = fmaf(W[P_V2 + k], rs_tanh(t[k]), v0);
            v1 = fmaf(W[P_V2 + k + 1], rs_tanh(t[k + 1]), v1);
        }
        if (live) a_.value[e] = v0 + v1;
    }
    // ---- policy head, log-softmax, inverse-CDF draw
    if (a_.logits || a_.act || a_.logp) {
        float t[HD];
#pragma unroll
        for (int o = 0; o < HD; ++o) t[o] = W[P_B1 + o];
        mv<GH, HD>(W + P_W1, [&](int k) -> float { return h[k]; }, t);
#pragma unroll
        for (int o = 0; o < HD; ++o) t[o] = rs_tanh(t[o]);
        float lg[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) lg[o] = W[P_B2 + o];
        mv<HD, 16>(W + P_W2, [&](int k) -> float { return t[k]; }, lg);
        if (a_.logits && live) {
#pragma unroll
            for (int o = 0; o < NA; o += 4) *reinterpret_cast<float4*>(a_.logits + (size_t)e * NA + o) = make_float4(lg[o], lg[o + 1], lg[o + 2], lg[o + 3]);
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
}

// The three kernels of this file carry the same GRU cell, heads and draw (the draw: csrc/rs_action.hpp's text), kept in step by hand.
// Shared as small inline pieces (cell, value head, policy head, draw) the arithmetic and the bits were the same, but two of the three
// fell outside the timing rule against their own copies (profiles/policy_pieces_timing.txt): K14 went from 195 to 197 VGPRs and eight
// launches at 1000 lanes timed 0.1578 ms against 0.1573 ms + 0.0004 ms of spread (five alternated rounds), rs_rnn_team_collect_kernel's
// bootstrap round at 4096 envs 0.0136 ms against 0.0135 ms + 0.0000 ms (three rounds).  rs_rnn_team_step_kernel stayed inside its
// spread, and has no partner left to share with.
//
// The policy round of a whole team in one launch: grid = (64-lane groups, agent), blockIdx.y's agent works on its rows of
// x [N][A][11], loc [N][A][2], u [N][A] and act8 [N][A] with its own weights and its own slab of h [A][N][24], updated in place (a
// lane has its row in registers before it stores).  K14's arithmetic, operation by operation and in K14's order, for the outputs an
// evaluation keeps -- the new state and the drawn action; no value head, no log-probability.  A body of its own, not K14's shared:
// with the body shared K14's code moved (298 -> 300 SGPR spills) and this kernel kept 14 SGPR spills; here a lane turns its row
// addresses and its uniform into vector registers before the products, whose weight stream needs the scalar file.
struct TeamArgs {
    const float* w[RS_MAX_AGENTS];   // the weight pointers travel in the argument block (8 x 8 bytes)
    const float* x;
    const float* loc;
    float* h;
    const float* u;
    const uint8_t* active;
    int8_t* act8;
    int N, A;
};

__global__ void __launch_bounds__(64) rs_rnn_team_step_kernel(TeamArgs t) {
    const int e = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y;
    const bool live = e < t.N && t.active[e] != 0;
    if (!__any(live)) return;
    const int ec = e < t.N ? e : t.N - 1;                  // idle lanes shadow a real lane, store nothing
    const cmem_t W = as_cmem(t.w[a]);
    const size_t i = (size_t)ec * t.A + a;
    float* hrow = t.h + ((size_t)a * t.N + ec) * GH;
    int8_t* arow = t.act8 + i;
    const float uu = t.u[i];
    int keep = live ? 1 : 0;                               // the lane's flag and its action's address in vector registers now: neither a
    asm volatile("" : "+v"(keep), "+v"(arow));             // mask pair nor the argument block's address is held across the products
    float x[NX], h[GH];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) x[k] = t.x[i * RS_OBS_DIM + k];
    x[RS_OBS_DIM] = t.loc[i * 2]; x[RS_OBS_DIM + 1] = t.loc[i * 2 + 1];
#pragma unroll
    for (int u = 0; u < GH; u += 4) {
        const float4 v = *reinterpret_cast<const float4*>(hrow + u);
        h[u] = v.x; h[u + 1] = v.y; h[u + 2] = v.z; h[u + 3] = v.w;
    }
    float gi[80], gh[80];
#pragma unroll
    for (int o = 0; o < 80; ++o) { gi[o] = W[P_BIH + o]; gh[o] = W[P_BHH + o]; }
    mv<NX, 80, 72>(W + P_IH, [&](int k) -> float { return x[k]; }, gi);
    mv<GH, 80, 72>(W + P_HH, [&](int k) -> float { return h[k]; }, gh);
#pragma unroll
    for (int j = 0; j < GH; ++j) {
        const float r = rs_sigmoid(gi[j] + gh[j]);
        const float z = rs_sigmoid(gi[GH + j] + gh[GH + j]);
        const float n = rs_tanh(gi[2 * GH + j] + r * gh[2 * GH + j]);
        h[j] = (1.0f - z) * n + z * h[j];
    }
    if (keep) {
#pragma unroll
        for (int u = 0; u < GH; u += 4) *reinterpret_cast<float4*>(hrow + u) = make_float4(h[u], h[u + 1], h[u + 2], h[u + 3]);
    }
    // ---- policy head, log-softmax, inverse-CDF draw
    float tt[HD];
#pragma unroll
    for (int o = 0; o < HD; ++o) tt[o] = W[P_B1 + o];
    mv<GH, HD>(W + P_W1, [&](int k) -> float { return h[k]; }, tt);
#pragma unroll
    for (int o = 0; o < HD; ++o) tt[o] = rs_tanh(tt[o]);
    float lg[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) lg[o] = W[P_B2 + o];
    mv<HD, 16>(W + P_W2, [&](int k) -> float { return tt[k]; }, lg);
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NA; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NA; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
    float cdf = 0.0f;
    int act = 0;
#pragma unroll
    for (int o = 0; o < NA; ++o) {
        const float lp = (lg[o] - mx) - lse;
        cdf += expf(lp);
        if (o < NA - 1 && cdf <= uu) { act = o + 1; }
    }
    if (keep) *arow = (int8_t)act;
}

// The policy round of 'bpf-a2c' (algos/test_environment/eval/test_policy.py:136-154) for every agent of every lane in one launch: the
// trained actor fed the bootstrap particle filter's location estimate in place of the PFGRU's.  The grid, the rows and the in-place h
// of rs_rnn_team_step_kernel; in front of its arithmetic a lane standardises and clips its reading (:400, 422) and scales the filter's
// estimate by the search area (:141), behind it the detector's position after the drawn move by the controller's own table (:18-27,
// 241).  K14's arithmetic, operation by operation and in K14's order, in between; a body of its own for the reason given above.  A
// finished lane gets act8 = 8 and nothing else of it is written.  Everything a lane needs after the products -- its flag, its
// addresses, its position -- is in vector registers before them.
struct BpfA2cArgs {
    const float* w[RS_MAX_AGENTS];
    const float* obs;      // [N][A][11] the raw observation
    const double* mean;    // [N][A] the reading's running mean and deviation (rs_welford.hpp)
    const double* sd;
    const double* est;     // [N][A][3] the filter's xpHatMean
    float* h;              // [A][N][24]
    const float* u;        // [N][A]
    const uint8_t* alive;  // [N]
    int8_t* act8;          // [N][A]
    const int* ax;         // [A][N] the env's detector positions
    const int* ay;
    double* sim_pos;       // [N][A][2]
    float* x_out;          // [N][A][11] or null
    float* loc_out;        // [N][A][2] or null
    double area_max;
    int N, A;
};

__global__ void __launch_bounds__(64) rs_bpf_a2c_step_kernel(BpfA2cArgs t) {
    const int e = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y;
    const bool live = e < t.N && t.alive[e] != 0;
    if (e < t.N && !live) t.act8[(size_t)e * t.A + a] = (int8_t)8;     // a finished lane idles
    if (!__any(live)) return;
    const int ec = e < t.N ? e : t.N - 1;                  // idle lanes shadow a real lane, store nothing
    const cmem_t W = as_cmem(t.w[a]);
    const size_t i = (size_t)ec * t.A + a;
    float* hrow = t.h + ((size_t)a * t.N + ec) * GH;
    int8_t* arow = t.act8 + i;
    double* srow = t.sim_pos + i * 2;
    const float uu = t.u[i];
    int px = t.ax[(size_t)a * t.N + ec], py = t.ay[(size_t)a * t.N + ec];
    int keep = live ? 1 : 0;
    float x[NX], h[GH];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) x[k] = t.obs[i * RS_OBS_DIM + k];
    // rs_welford_standardized's expression, then np.clip(., -8, 8)
    x[0] = fminf(fmaxf((float)(((double)x[0] - t.mean[i]) / t.sd[i]), -8.0f), 8.0f);
    x[RS_OBS_DIM] = (float)(t.est[i * 3 + 1] / t.area_max); x[RS_OBS_DIM + 1] = (float)(t.est[i * 3 + 2] / t.area_max);
    if (keep) {
        if (t.x_out) {
#pragma unroll
            for (int k = 0; k < RS_OBS_DIM; ++k) t.x_out[i * RS_OBS_DIM + k] = x[k];
        }
        if (t.loc_out) { t.loc_out[i * 2] = x[RS_OBS_DIM]; t.loc_out[i * 2 + 1] = x[RS_OBS_DIM + 1]; }
    }
    asm volatile("" : "+v"(keep), "+v"(arow), "+v"(srow), "+v"(px), "+v"(py));
#pragma unroll
    for (int u = 0; u < GH; u += 4) {
        const float4 v = *reinterpret_cast<const float4*>(hrow + u);
        h[u] = v.x; h[u + 1] = v.y; h[u + 2] = v.z; h[u + 3] = v.w;
    }
    float gi[80], gh[80];
#pragma unroll
    for (int o = 0; o < 80; ++o) { gi[o] = W[P_BIH + o]; gh[o] = W[P_BHH + o]; }
    mv<NX, 80, 72>(W + P_IH, [&](int k) -> float { return x[k]; }, gi);
    mv<GH, 80, 72>(W + P_HH, [&](int k) -> float { return h[k]; }, gh);
#pragma unroll
    for (int j = 0; j < GH; ++j) {
        const float r = rs_sigmoid(gi[j] + gh[j]);
        const float z = rs_sigmoid(gi[GH + j] + gh[GH + j]);
        const float n = rs_tanh(gi[2 * GH + j] + r * gh[2 * GH + j]);
        h[j] = (1.0f - z) * n + z * h[j];
    }
    if (keep) {
#pragma unroll
        for (int u = 0; u < GH; u += 4) *reinterpret_cast<float4*>(hrow + u) = make_float4(h[u], h[u + 1], h[u + 2], h[u + 3]);
    }
    // ---- policy head, log-softmax, inverse-CDF draw
    float tt[HD];
#pragma unroll
    for (int o = 0; o < HD; ++o) tt[o] = W[P_B1 + o];
    mv<GH, HD>(W + P_W1, [&](int k) -> float { return h[k]; }, tt);
#pragma unroll
    for (int o = 0; o < HD; ++o) tt[o] = rs_tanh(tt[o]);
    float lg[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) lg[o] = W[P_B2 + o];
    mv<HD, 16>(W + P_W2, [&](int k) -> float { return tt[k]; }, lg);
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NA; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NA; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
    float cdf = 0.0f;
    int act = 0;
#pragma unroll
    for (int o = 0; o < NA; ++o) {
        const float lp = (lg[o] - mx) - lse;
        cdf += expf(lp);
        if (o < NA - 1 && cdf <= uu) { act = o + 1; }
    }
    if (keep) {
        // ACTION (test_policy.py:18-27): 0 (-100, 0), 1 (-71, 71), 2 (0, 100), 3 (71, 71), 4 (100, 0), 5 (71, -71), 6 (0, -100), 7 (-71, -71)
        const double dx = act == 0 ? -100.0 : (act == 1 || act == 7) ? -71.0 : (act == 2 || act == 6) ? 0.0 : act == 4 ? 100.0 : 71.0;
        const double dy = (act == 0 || act == 4) ? 0.0 : (act == 1 || act == 3) ? 71.0 : act == 2 ? 100.0 : act == 6 ? -100.0 : -71.0;
        *arow = (int8_t)act;
        srow[0] = (double)px + dx; srow[1] = (double)py + dy;
    }
}

// The policy round of a whole team as a collector runs it, step round (u given) or bootstrap round (u null), in one launch: the grid,
// the rows and the in-place h of rs_rnn_team_step_kernel, with K14's value head and log-probability and an optional mask.  The step
// round stores h, the action (act [A][N] int64 and / or act8 [N][A]) and, when f = logp_val_boot [A][3][N] is given, the log-
// probability (slot 0) and the value (slot 1); the bootstrap round stores the value of the GRU's next state (slot 2) and nothing else.
// K14's arithmetic, operation by operation and in K14's order; a body of its own for the reason given above.  Every address a lane
// stores through is in vector registers before the products; the two round switches are re-read from the argument block.
struct CollectArgs {
    const float* w[RS_MAX_AGENTS];
    const float* x;
    const float* loc;
    float* h;
    const float* u;        // [N][A] or null: the bootstrap round
    int64_t* act;          // [A][N] or null
    float* f;              // [A][3][N] (logp, value, bootstrap value) or null
    int8_t* act8;          // [N][A] or null
    const uint8_t* mask;   // [N] or null
    int N, A;
};

__global__ void __launch_bounds__(64) rs_rnn_team_collect_kernel(CollectArgs t) {
    const int e = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y;
    const bool live = e < t.N && (t.mask == nullptr || t.mask[e] != 0);
    if (!__any(live)) return;
    const int ec = e < t.N ? e : t.N - 1;                  // idle lanes shadow a real lane, store nothing
    const cmem_t W = as_cmem(t.w[a]);
    const size_t i = (size_t)ec * t.A + a;
    const bool step = t.u != nullptr;
    float* hrow = t.h + ((size_t)a * t.N + ec) * GH;
    float* frow = t.f ? t.f + (size_t)a * 3 * t.N + ec : nullptr;          // slot s of this lane: frow[s N]
    float* vrow = frow ? frow + (size_t)(step ? 1 : 2) * t.N : nullptr;
    int8_t* arow = t.act8 ? t.act8 + i : nullptr;
    int64_t* krow = t.act ? t.act + (size_t)a * t.N + ec : nullptr;
    const float uu = step ? t.u[i] : 0.0f;
    int keep = live ? 1 : 0;
    asm volatile("" : "+v"(keep), "+v"(frow), "+v"(vrow), "+v"(arow), "+v"(krow));
    float x[NX], h[GH];
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) x[k] = t.x[i * RS_OBS_DIM + k];
    x[RS_OBS_DIM] = t.loc[i * 2]; x[RS_OBS_DIM + 1] = t.loc[i * 2 + 1];
#pragma unroll
    for (int u = 0; u < GH; u += 4) {
        const float4 v = *reinterpret_cast<const float4*>(hrow + u);
        h[u] = v.x; h[u + 1] = v.y; h[u + 2] = v.z; h[u + 3] = v.w;
    }
    float gi[80], gh[80];
#pragma unroll
    for (int o = 0; o < 80; ++o) { gi[o] = W[P_BIH + o]; gh[o] = W[P_BHH + o]; }
    mv<NX, 80, 72>(W + P_IH, [&](int k) -> float { return x[k]; }, gi);
    mv<GH, 80, 72>(W + P_HH, [&](int k) -> float { return h[k]; }, gh);
#pragma unroll
    for (int j = 0; j < GH; ++j) {
        const float r = rs_sigmoid(gi[j] + gh[j]);
        const float z = rs_sigmoid(gi[GH + j] + gh[GH + j]);
        const float n = rs_tanh(gi[2 * GH + j] + r * gh[2 * GH + j]);
        h[j] = (1.0f - z) * n + z * h[j];
    }
    if (t.u != nullptr && keep) {
#pragma unroll
        for (int u = 0; u < GH; u += 4) *reinterpret_cast<float4*>(hrow + u) = make_float4(h[u], h[u + 1], h[u + 2], h[u + 3]);
    }
    // ---- value head
    if (t.f != nullptr) {
        float tv[HD];
#pragma unroll
        for (int o = 0; o < HD; ++o) tv[o] = W[P_VB1 + o];
        mv<GH, HD>(W + P_V1, [&](int k) -> float { return h[k]; }, tv);
        float v0 = W[P_V2 + HD], v1 = 0.0f;
#pragma unroll
        for (int k = 0; k < HD; k += 2) {
            v0 = fmaf(W[P_V2 + k], rs_tanh(tv[k]), v0);
            v1 = fmaf(W[P_V2 + k + 1], rs_tanh(tv[k + 1]), v1);
        }
        if (keep) *vrow = v0 + v1;
    }
    if (t.u == nullptr) return;
    // ---- policy head, log-softmax, inverse-CDF draw
    float tt[HD];
#pragma unroll
    for (int o = 0; o < HD; ++o) tt[o] = W[P_B1 + o];
    mv<GH, HD>(W + P_W1, [&](int k) -> float { return h[k]; }, tt);
#pragma unroll
    for (int o = 0; o < HD; ++o) tt[o] = rs_tanh(tt[o]);
    float lg[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) lg[o] = W[P_B2 + o];
    mv<HD, 16>(W + P_W2, [&](int k) -> float { return tt[k]; }, lg);
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NA; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NA; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
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
    if (keep) {
        if (krow) *krow = act;
        if (arow) *arow = (int8_t)act;
        if (frow) *frow = lp_sel;
    }
}

// out[k] += sum_o W[k][o] c(o) on a k-major [K][OUTP] block (the transposed product: a dot product along each row)
template <int K, int OUTP, typename F>
__device__ __forceinline__ void mvt(cmem_t W, F cval, float (&out)[K]) { rs_ss_mvt<K, OUTP>(W, cval, out); }

// K15: heads, per-sample PPO-clip / value loss and their back-propagation for every (step, episode) sample of an episode chunk:
// update_rada2c's loss (algos/multiagent/ppo.py:1191-1234) behind the GRU.  One sample per lane.  Writes dL/dh (the input of K12's
// backward), the per-sample factors of the head weight gradients (the caller reduces the outer products with batched GEMMs) and
// per-wave partial sums of the statistics.  The loss derivative is K7's (csrc/rs_ppo_grad2.hpp), pinned to the reference there.
struct HeadArgs {
    const float* w;        // packed policy weights (K14 layout; the head blocks are used)
    const float* hs;       // [S][24]
    const int64_t* act;    // [S]
    const float* adv;      // [S]
    const float* ret;      // [S]
    const float* lpo;      // [S] log-probability at collection time
    const float* wt;       // [S] sample weight (0 on padded steps)
    float* dhs;            // [S][24]
    float* dfac;           // [S][80]: d pre-tanh (policy head) [32] | d pre-tanh (value head) [32] | d logits [8] | d value | 0 x 7
    float* tfac;           // [S][64]: tanh (policy head) [32] | tanh (value head) [32]
    float* stats;          // [waves][8]: kl, entropy, clip fraction, value loss, surrogate, weight sum, 0, 0 (weighted sums)
    long long S;
    float clip, vf_coef;
};

__global__ void __launch_bounds__(64) rs_a2c_heads_kernel(HeadArgs a_) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < a_.S;
    const long long ic = live ? i : a_.S - 1;
    const cmem_t W = as_cmem(a_.w);
    float h[GH];
#pragma unroll
    for (int u = 0; u < GH; u += 4) {
        const float4 v = *reinterpret_cast<const float4*>(a_.hs + ic * GH + u);
        h[u] = v.x; h[u + 1] = v.y; h[u + 2] = v.z; h[u + 3] = v.w;
    }
    const float wi = live ? a_.wt[ic] : 0.0f;
    const int a = (int)a_.act[ic];
    const float adv = a_.adv[ic], ret = a_.ret[ic], lpo = a_.lpo[ic];
    float tp[HD], tv[HD];
#pragma unroll
    for (int o = 0; o < HD; ++o) { tp[o] = W[P_B1 + o]; tv[o] = W[P_VB1 + o]; }
    mv<GH, HD>(W + P_W1, [&](int k) -> float { return h[k]; }, tp);
    mv<GH, HD>(W + P_V1, [&](int k) -> float { return h[k]; }, tv);
#pragma unroll
    for (int o = 0; o < HD; ++o) { tp[o] = rs_tanh(tp[o]); tv[o] = rs_tanh(tv[o]); }
    float lg[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) lg[o] = W[P_B2 + o];
    mv<HD, 16>(W + P_W2, [&](int k) -> float { return tp[k]; }, lg);
    float v0 = W[P_V2 + HD], v1 = 0.0f;
#pragma unroll
    for (int k = 0; k < HD; k += 2) {
        v0 = fmaf(W[P_V2 + k], tv[k], v0);
        v1 = fmaf(W[P_V2 + k + 1], tv[k + 1], v1);
    }
    const float val = v0 + v1;
    // ---- per-sample loss terms and derivative (K7's formulas)
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
    float dl[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) dl[j] = j < NA ? g_lp * (((a == j) ? 1.0f : 0.0f) - pj[j < NA ? j : 0]) : 0.0f;
    const float diff = val - ret;
    const float dval = 2.0f * a_.vf_coef * wi * diff;
    // ---- back through the heads
    float dp[HD], dv[HD];
#pragma unroll
    for (int k = 0; k < HD; ++k) dp[k] = 0.0f;
    // the backward products read the same rows as the forward ones: a laundered pointer keeps GVN from holding (and spilling) them
    auto wptr = [&]() -> cmem_t { const float* w = a_.w; asm volatile("" : "+s"(w)); return as_cmem(w); };
    mvt<HD, 16>(wptr() + P_W2, [&](int o) -> float { return dl[o]; }, dp);
#pragma unroll
    for (int k = 0; k < HD; ++k) {
        dp[k] = dp[k] * (1.0f - tp[k] * tp[k]);
        dv[k] = wptr()[P_V2 + k] * dval * (1.0f - tv[k] * tv[k]);
    }
    float dh[GH];
#pragma unroll
    for (int j = 0; j < GH; ++j) dh[j] = 0.0f;
    mvt<GH, HD>(wptr() + P_W1, [&](int k) -> float { return dp[k]; }, dh);
    mvt<GH, HD>(wptr() + P_V1, [&](int k) -> float { return dv[k]; }, dh);
    if (live) {
        float* o = a_.dhs + i * GH;
#pragma unroll
        for (int u = 0; u < GH; u += 4) *reinterpret_cast<float4*>(o + u) = make_float4(dh[u], dh[u + 1], dh[u + 2], dh[u + 3]);
        float* d = a_.dfac + i * 80;
#pragma unroll
        for (int u = 0; u < HD; u += 4) {
            *reinterpret_cast<float4*>(d + u) = make_float4(dp[u], dp[u + 1], dp[u + 2], dp[u + 3]);
            *reinterpret_cast<float4*>(d + HD + u) = make_float4(dv[u], dv[u + 1], dv[u + 2], dv[u + 3]);
        }
        *reinterpret_cast<float4*>(d + 64) = make_float4(dl[0], dl[1], dl[2], dl[3]);
        *reinterpret_cast<float4*>(d + 68) = make_float4(dl[4], dl[5], dl[6], dl[7]);
        *reinterpret_cast<float4*>(d + 72) = make_float4(dval, 0.0f, 0.0f, 0.0f);
        *reinterpret_cast<float4*>(d + 76) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float* t = a_.tfac + i * 64;
#pragma unroll
        for (int u = 0; u < HD; u += 4) {
            *reinterpret_cast<float4*>(t + u) = make_float4(tp[u], tp[u + 1], tp[u + 2], tp[u + 3]);
            *reinterpret_cast<float4*>(t + HD + u) = make_float4(tv[u], tv[u + 1], tv[u + 2], tv[u + 3]);
        }
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

extern "C" {

int rs_a2c_heads_loss(const float* weights, const float* hs, const int64_t* act, const float* adv, const float* ret, const float* logp_old,
                      const float* sample_weight, float* dhs, float* dfac, float* tfac, float* stats, int64_t samples, double clip_ratio,
                      double vf_coef, rs_stream_t stream) {
    if (!weights || !hs || !act || !adv || !ret || !logp_old || !sample_weight || !dhs || !dfac || !tfac || !stats || samples < 1)
        return RS_ERR_INVALID_ARG;
    HeadArgs a{weights, hs, act, adv, ret, logp_old, sample_weight, dhs, dfac, tfac, stats, (long long)samples, (float)clip_ratio, (float)vf_coef};
    hipLaunchKernelGGL(rs_a2c_heads_kernel, dim3((unsigned)((samples + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_rnn_policy_step(const float* weights, const float* x, const float* loc, const float* h, const float* u, float* h_out,
                       float* logits, float* value, int64_t* act, float* logp, int32_t num_envs, rs_stream_t stream) {
    if (!weights || !x || !loc || !h || num_envs < 1) return RS_ERR_INVALID_ARG;
    if ((act || logp) && !u) return RS_ERR_INVALID_ARG;
    PolArgs a{weights, x, loc, h, u, h_out, logits, value, act, logp, num_envs, RS_OBS_DIM, 2, 1, nullptr, 1, nullptr};
    hipLaunchKernelGGL(rs_rnn_policy_kernel, dim3((num_envs + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_rnn_policy_step_rows(const float* weights, const float* x, int32_t x_stride, const float* loc, int32_t loc_stride, const float* h,
                            const float* u, int32_t u_stride, float* h_out, float* value, int64_t* act, float* logp, int8_t* act8,
                            int32_t act8_stride, const uint8_t* mask, int32_t num_envs, rs_stream_t stream) {
    if (!weights || !x || !loc || !h || num_envs < 1 || x_stride < RS_OBS_DIM || loc_stride < 2 || u_stride < 1 || act8_stride < 1)
        return RS_ERR_INVALID_ARG;
    if ((act || logp || act8) && !u) return RS_ERR_INVALID_ARG;
    PolArgs a{weights, x, loc, h, u, h_out, nullptr, value, act, logp, num_envs, x_stride, loc_stride, u_stride, act8, act8_stride, mask};
    hipLaunchKernelGGL(rs_rnn_policy_kernel, dim3((num_envs + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_rnn_team_eval_step(const float* const* weights, int32_t num_agents, const float* x, const float* loc, float* h, const float* u,
                          const uint8_t* active, int8_t* act8, int32_t num_envs, rs_stream_t stream) {
    if (!weights || !x || !loc || !h || !u || !active || !act8 || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_envs < 1)
        return RS_ERR_INVALID_ARG;
    TeamArgs t{};
    for (int a = 0; a < RS_MAX_AGENTS; ++a) {
        if (a < num_agents && !weights[a]) return RS_ERR_INVALID_ARG;
        t.w[a] = weights[a < num_agents ? a : 0];                  // the slots behind the team repeat agent 0 (never read)
    }
    t.x = x; t.loc = loc; t.h = h; t.u = u; t.active = active; t.act8 = act8; t.N = num_envs; t.A = num_agents;
    hipLaunchKernelGGL(rs_rnn_team_step_kernel, dim3((num_envs + 63) / 64, num_agents), dim3(64), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_bpf_a2c_eval_step(rs_handle* h, const float* const* weights, int32_t num_agents, const float* obs, const double* mean, const double* std,
                         const double* est, double area_max, float* hid, const float* u, const uint8_t* alive, int8_t* act8, double* sim_pos,
                         float* x_out, float* loc_out, rs_stream_t stream) {
    if (!h || !weights || !obs || !mean || !std || !est || !hid || !u || !alive || !act8 || !sim_pos) return RS_ERR_INVALID_ARG;
    if (num_agents < 1 || num_agents > RS_MAX_AGENTS || num_agents != h->P.A) return RS_ERR_INVALID_ARG;
    BpfA2cArgs t{};
    for (int a = 0; a < RS_MAX_AGENTS; ++a) {
        if (a < num_agents && !weights[a]) return RS_ERR_INVALID_ARG;
        t.w[a] = weights[a < num_agents ? a : 0];                  // the slots behind the team repeat agent 0 (never read)
    }
    t.obs = obs; t.mean = mean; t.sd = std; t.est = est; t.h = hid; t.u = u; t.alive = alive; t.act8 = act8;
    t.ax = h->P.ax; t.ay = h->P.ay; t.sim_pos = sim_pos; t.x_out = x_out; t.loc_out = loc_out; t.area_max = area_max;
    t.N = h->P.N; t.A = num_agents;
    hipLaunchKernelGGL(rs_bpf_a2c_step_kernel, dim3((t.N + 63) / 64, num_agents), dim3(64), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_rnn_team_step(const float* const* weights, int32_t num_agents, const float* x, const float* loc, float* h, const float* u, int64_t* act,
                     float* logp_val_boot, int8_t* act8, const uint8_t* mask, int32_t num_envs, rs_stream_t stream) {
    if (!weights || !x || !loc || !h || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_envs < 1) return RS_ERR_INVALID_ARG;
    if (u ? (!act && !act8) : !logp_val_boot) return RS_ERR_INVALID_ARG;       // a step round draws an action, a bootstrap round a value
    CollectArgs t{};
    for (int a = 0; a < RS_MAX_AGENTS; ++a) {
        if (a < num_agents && !weights[a]) return RS_ERR_INVALID_ARG;
        t.w[a] = weights[a < num_agents ? a : 0];                  // the slots behind the team repeat agent 0 (never read)
    }
    t.x = x; t.loc = loc; t.h = h; t.u = u; t.act = act; t.f = logp_val_boot; t.act8 = act8; t.mask = mask; t.N = num_envs; t.A = num_agents;
    hipLaunchKernelGGL(rs_rnn_team_collect_kernel, dim3((num_envs + 63) / 64, num_agents), dim3(64), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

// rs_draws.hip -- the cold kernels of the draw contract (csrc/rs_draws.hpp), one copy each with the width as an argument: fresh
// particle sets for the envs that begin an episode, the draws of a training pass as buffers, the GRU's initial state.  The default
// exports (24 units) and the width-taking ones are wrappers around the same kernel; each keeps its own argument checks.
//
// HC, where a kernel has it: the width at compile time, the loops over a lane's units unrolled; 0: the width is the argument.  The
// default reset and draws exports launch the 24-unit instantiation: through the runtime loops they were slower than before there was
// one copy (reset of 4096 envs x 4 owners 20.0 against 18.7 us, draws of 8192 episodes x 120 steps 1087 against 1077 us:
// profiles/draw_contract_refactor_ab.txt); the width-taking exports launch <0> at every width, 24 included.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_draws.hpp"

namespace {

constexpr int P = RS_PFGRU_PARTICLES;
bool pf_width_ok(int H) { return H >= 8 && H <= 64 && H % 8 == 0; }

// f(u) for the units u = 0, STEP, .. below the width
template <int HC, int STEP, typename F>
__device__ __forceinline__ void for_units(int H, F f) {
    if constexpr (HC > 0) {
#pragma unroll
        for (int u = 0; u < HC; u += STEP) f(u);
    } else {
        for (int u = 0; u < H; u += STEP) f(u);
    }
}

// reset_hidden (RADTEAM_core.py:2030-2033) for the masked envs: h0 ~ U[0,1) from the hash (kind 0), p0 = log(1 / P).
// One lane per (owner, env, particle); the caller has already advanced episode[] and zeroed calls[] for those envs.
template <int HC>
__global__ void __launch_bounds__(256) rs_pfgru_reset_kernel(float* h, float* p, const int64_t* base, const int64_t* episode,
                                                             const int64_t* calls, const uint8_t* mask, int N, int A, int H_) {
    const int H = HC ? HC : H_;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A * N * P) return;
    const int pl = (int)(i % P);
    const long long slot = i / P;
    const int n = (int)(slot % N);
    if (mask && !mask[n]) return;
    const uint64_t pk = rs_draw_lane(rs_draw_key(rs_draw_base(base[slot]), rs_draw_counter(episode[n], calls[n])), pl);
    float4* hw = reinterpret_cast<float4*>(h + slot * P * H) + pl;                 // quad-major, as the step kernels read it
    for_units<HC, 4>(H, [&](int u) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)rs_hash_uniform(pk + (uint64_t)(u + j));
        hw[(u / 4) * P] = make_float4(v[0], v[1], v[2], v[3]);
    });
    p[i] = RS_LOG_INV_P;
}

// The draws of one training pass over an episode-major batch (rada2c.HashDraws) in one launch instead of ~25 int64 element-wise
// launches per step: key[e] -> h0 [E][P][H] (uniforms, kind 0), eps [L][E][P][H] (standard normals, kind 1, step t) and
// u [L][E][P] (resampling uniforms, kind 2, step t).  One lane per (t, episode, particle).  The normals are evaluated as the step
// kernels evaluate them (rs_hash_normal_pair): with the library logf / cosf this kernel was instruction bound at a quarter of the
// HBM fill rate
template <int HC>
__global__ void __launch_bounds__(256) rs_pfgru_draws_kernel(const int64_t* __restrict__ key, int E, int L, int H_, float* __restrict__ h0,
                                                             float* __restrict__ eps, double* __restrict__ u) {
    const int H = HC ? HC : H_;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)L * E * P) return;
    const int pl = (int)(i % P);
    const long long te = i / P;
    const int e = (int)(te % E), t = (int)(te / E);
    const uint64_t kb = rs_draw_base(key[e]);
    const uint64_t k1 = rs_draw_lane(rs_draw_key(kb, (uint64_t)(t * 8 + 1)), pl);
    float* ew = eps + i * H;
    for_units<HC, 4>(H, [&](int q) {
        float v[4];
        rs_hash_normal_pair(rs_hash_bits(k1 + (uint64_t)q), v[0], v[1]);
        rs_hash_normal_pair(rs_hash_bits(k1 + (uint64_t)(q + 2)), v[2], v[3]);
        *reinterpret_cast<float4*>(ew + q) = make_float4(v[0], v[1], v[2], v[3]);
    });
    u[i] = rs_hash_uniform(rs_draw_lane(rs_draw_key(kb, (uint64_t)(t * 8 + 2)), pl));
    if (t == 0) {
        const uint64_t k0 = rs_draw_lane(rs_draw_key(kb, 0), pl);                 // kind 0, step 0
        float* hw = h0 + ((long long)e * P + pl) * H;
        for_units<HC, 1>(H, [&](int q) { hw[q] = (float)rs_hash_uniform(k0 + (uint64_t)q); });
    }
}

// _get_init_states (RADA2C_core.py:458-461) for the envs that begin an episode: h0 ~ U(-scale, scale) from the counter hash
// (kind 5 of the env's key, counter = episodes_begun[n]); one lane per (agent, env, unit).  The torch composition of the
// same hash was ~30 int64 element-wise launches per lock-step of the collector.
__global__ void __launch_bounds__(256) rs_gru_h0_kernel(float* __restrict__ h, const int64_t* __restrict__ base, const int64_t* __restrict__ begun,
                                                        const uint8_t* __restrict__ mask, float scale, int hid, int N, int A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A * N * hid) return;
    const int j = (int)(i % hid);
    const long long slot = i / hid;
    const int n = (int)(slot % N);
    if (mask && !mask[n]) return;
    const uint64_t key = rs_draw_key(rs_draw_base(base[slot]), (uint64_t)begun[n] * 8ull + 5ull);
    const double u = rs_hash_uniform(rs_draw_lane(key, 0) + (uint64_t)j);
    h[i] = ((float)u * 2.0f - 1.0f) * scale;
}

template <int HC>
int launch_reset(float* h, float* p, const int64_t* base_key, const int64_t* episode, const int64_t* calls, const uint8_t* mask, int N, int A,
                 int H, rs_stream_t stream) {
    const long long lanes = (long long)N * A * P;
    hipLaunchKernelGGL(rs_pfgru_reset_kernel<HC>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       h, p, base_key, episode, calls, mask, N, A, H);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

template <int HC>
int launch_draws(const int64_t* keys, int E, int L, int H, float* h0, float* eps, double* u, rs_stream_t stream) {
    const long long lanes = (long long)L * E * P;
    hipLaunchKernelGGL(rs_pfgru_draws_kernel<HC>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), keys,
                       E, L, H, h0, eps, u);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int launch_h0(float* h, const int64_t* base_key, const int64_t* begun, const uint8_t* mask, double scale, int hid, int N, int A,
              rs_stream_t stream) {
    const long long lanes = (long long)N * A * hid;
    hipLaunchKernelGGL(rs_gru_h0_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), h, base_key,
                       begun, mask, (float)scale, hid, N, A);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // namespace

extern "C" {

int rs_pfgru_reset(float* h, float* p, const int64_t* base_key, const int64_t* episode, const int64_t* calls, const uint8_t* mask,
                   int32_t num_envs, int32_t num_agents, rs_stream_t stream) {
    if (!h || !p || !base_key || !episode || !calls || num_envs < 1 || num_agents < 1) return RS_ERR_INVALID_ARG;
    return launch_reset<RS_PFGRU_HIDDEN>(h, p, base_key, episode, calls, mask, num_envs, num_agents, RS_PFGRU_HIDDEN, stream);
}

int rs_pfgru_sized_reset(float* h, float* p, const int64_t* base_key, const int64_t* episode, const int64_t* calls, const uint8_t* mask,
                         int32_t num_envs, int32_t num_agents, int32_t hidden, rs_stream_t stream) {
    if (!pf_width_ok(hidden)) return RS_ERR_UNSUPPORTED;
    if (!h || !p || !base_key || !episode || !calls || num_envs < 1 || num_agents < 1 || num_agents > RS_MAX_AGENTS) return RS_ERR_INVALID_ARG;
    return launch_reset<0>(h, p, base_key, episode, calls, mask, num_envs, num_agents, hidden, stream);
}

int rs_pfgru_draws(const int64_t* keys, int32_t episodes, int32_t steps, float* h0, float* eps, double* u, rs_stream_t stream) {
    if (!keys || !h0 || !eps || !u || episodes < 1 || steps < 1) return RS_ERR_INVALID_ARG;
    return launch_draws<RS_PFGRU_HIDDEN>(keys, episodes, steps, RS_PFGRU_HIDDEN, h0, eps, u, stream);
}

int rs_pfgru_sized_draws(const int64_t* keys, int32_t episodes, int32_t steps, int32_t hidden, float* h0, float* eps, double* u,
                         rs_stream_t stream) {
    if (!pf_width_ok(hidden) || !keys || !h0 || !eps || !u || episodes < 0 || steps < 1) return RS_ERR_INVALID_ARG;
    if (episodes == 0) return RS_OK;
    return launch_draws<0>(keys, episodes, steps, hidden, h0, eps, u, stream);
}

int rs_gru_h0_reset(float* h, const int64_t* base_key, const int64_t* episodes_begun, const uint8_t* mask, double scale, int32_t num_envs,
                    int32_t num_agents, rs_stream_t stream) {
    if (!h || !base_key || !episodes_begun || num_envs < 1 || num_agents < 1) return RS_ERR_INVALID_ARG;
    return launch_h0(h, base_key, episodes_begun, mask, scale, RS_GRU_HIDDEN, num_envs, num_agents, stream);
}

int rs_gru_h0_reset_sized(float* h, const int64_t* base_key, const int64_t* episodes_begun, const uint8_t* mask, double scale, int32_t hid,
                          int32_t num_envs, int32_t num_agents, rs_stream_t stream) {
    if (hid < 1 || hid > 64) return RS_ERR_UNSUPPORTED;
    if (!h || !base_key || !episodes_begun || num_envs < 1 || num_agents < 1) return RS_ERR_INVALID_ARG;
    return launch_h0(h, base_key, episodes_begun, mask, scale, hid, num_envs, num_agents, stream);
}

}  // extern "C"

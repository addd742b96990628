// rs_draws.hpp -- the draw contract of the PFGRU and GRU kernels, stated once: the counter hash that replaces the reference's torch
// generator (the project's documented RNG deviation), the fast transcendentals its normals share with the cells, and the helpers of
// a 40-particle set.  Every kernel that draws includes this header; radiation_ppo_amd/pfgru.py is the same contract in torch, and
// the bit-identity tests hold the two to each other.
//
// A draw is hash(key): key = lane(draw_key(base, counter + kind), particle) + unit on wrapping 64-bit arithmetic.
//   base      rs_draw_base(k): k = the int64 identity of a stream -- PredictorBank._base[owner][env] for the collectors, the episode
//             key of a training pass (rada2c.HashDraws.k).  * 1000003 spreads neighbouring identities apart.
//   counter   when in the stream, a multiple of 8: rs_draw_counter(episode, calls) = (episode * 100003 + calls) * 8 for the collectors
//             (100003 > the calls of an episode: no two (episode, call) pairs meet), t * 8 for step t of a training pass,
//             episodes_begun * 8 for the GRU's initial state.
//   kind      what the draw is for, 0 .. 7 in the counter's low three bits: 0 initial particles (uniform), 1 reparameterisation noise
//             (normal pairs), 2 resampling uniforms, 3 the GRU h0 of a training pass (rada2c.HashDraws.gru_h0_u), 5 the collectors' GRU h0.
//   rs_draw_key(base, counter + kind) == pfgru.draw_key(k, counter + kind): the 64-bit odd multiplier separates counters before the
//             xor with the base.
//   lane      rs_draw_lane(key, particle) = key * 1048583 + particle * 4096; the unit (< 4096) is added by the caller (pfgru.lane_offsets).
//             The GRU's h0 has no particles: lane 0, unit j.
//   hash      rs_hash_bits == pfgru.hash_bits (splitmix64's finaliser); rs_hash_uniform == pfgru.hash_uniform (top 53 bits -> [0, 1));
//             rs_hash_normal_pair == pfgru.hash_normal (ONE hash per PAIR of units, keyed by the even unit: float32 Box-Muller).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"

static_assert(RS_PFGRU_PARTICLES == 40, "rs_max40 / rs_sum40 / rs_prefix40 / rs_search40 walk 40 particles");
constexpr float RS_LOG_INV_P = -3.6888794541139363f;               // float32(log(1 / 40)): a fresh particle's log weight

__device__ __forceinline__ uint64_t rs_hash_bits(uint64_t key) {
    uint64_t x = key * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ double rs_hash_uniform(uint64_t key) { return (double)(rs_hash_bits(key) >> 11) * (1.0 / 9007199254740992.0); }

__device__ __forceinline__ uint64_t rs_draw_base(int64_t k) { return (uint64_t)k * 1000003ull; }
__device__ __forceinline__ uint64_t rs_draw_counter(int64_t episode, int64_t calls) {
    return ((uint64_t)episode * 100003ull + (uint64_t)calls) * 8ull;
}
__device__ __forceinline__ uint64_t rs_draw_key(uint64_t base, uint64_t counter_kind) { return base ^ (counter_kind * 0xA24BAED4963EE407ull); }
__device__ __forceinline__ uint64_t rs_draw_lane(uint64_t key, int particle) { return key * 1048583ull + (uint64_t)particle * 4096ull; }

// the hash of an even unit's key -> the standard normals of that unit and the next: u1 in (0, 1] from bits 63..40, u2 in [0, 1) from
// bits 39..16, r = sqrt(-2 ln u1) (v_log_f32 is log2: -1.38629436 = -2 ln 2), cosine / sine of the turn u2 (v_cos_f32 / v_sin_f32
// take revolutions: no range reduction).  Hardware transcendentals, 1 ulp each: |error| ~ 1e-6 against pfgru.hash_normal
__device__ __forceinline__ void rs_hash_normal_pair(uint64_t hx, float& even, float& odd) {
    const float u1 = (float)((uint32_t)(hx >> 40) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)((uint32_t)(hx >> 16) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    const float r = __builtin_amdgcn_sqrtf(-1.38629436f * __builtin_amdgcn_logf(u1));
    even = r * __builtin_amdgcn_cosf(u2);
    odd = r * __builtin_amdgcn_sinf(u2);
}

// sigmoid, exp, log and tanh on v_exp_f32 / v_log_f32 / v_rcp_f32 (1 ulp each, branch free; the library expf / logf / IEEE division are
// 10-20 instructions each)
__device__ __forceinline__ float rs_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * x)); }
__device__ __forceinline__ float rs_exp(float x) { return __builtin_amdgcn_exp2f(1.44269504f * x); }
__device__ __forceinline__ float rs_log(float x) { return 0.69314718f * __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float rs_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008f * x)); }

// ---- a set's 40 values in LDS (16-byte aligned), reduced by every lane itself in index order: deterministic and independent of which
// sets share a workgroup
__device__ __forceinline__ float rs_max40(const float* v) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const float4 t = reinterpret_cast<const float4*>(v)[i];
        m = fmaxf(fmaxf(m, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
    }
    return m;
}
__device__ __forceinline__ float rs_sum40(const float* v) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const float4 t = reinterpret_cast<const float4*>(v)[i];
        s = (((s + t.x) + t.y) + t.z) + t.w;
    }
    return s;
}
// soft resampling's CDF at particle q is mine / run: the float64 prefix sum of the 40 weights up to q, in index order (torch.cumsum of
// the .double() weights), and their total.  The caller divides (IEEE: the quotient decides indices) and stores under its own lane
// predicate -- dividing or storing in here costs the sized step kernels an SGPR spill
__device__ __forceinline__ void rs_prefix40(const float* w, int q, double& mine, double& run) {
    run = 0.0; mine = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const float4 t = reinterpret_cast<const float4*>(w)[i];
        run += (double)t.x; mine = (4 * i == q) ? run : mine;
        run += (double)t.y; mine = (4 * i + 1 == q) ? run : mine;
        run += (double)t.z; mine = (4 * i + 2 == q) ? run : mine;
        run += (double)t.w; mine = (4 * i + 3 == q) ? run : mine;
    }
}
// torch.searchsorted(cdf, ru, right=True): the entries <= ru, counted (40 where rounding left cdf[39] below ru: the caller clamps)
__device__ __forceinline__ int rs_search40(const double* cdf, double ru) {
    int idx = 0;
#pragma unroll
    for (int j = 0; j < 20; ++j) {
        const double2 c2 = reinterpret_cast<const double2*>(cdf)[j];
        idx += (c2.x <= ru) ? 1 : 0;
        idx += (c2.y <= ru) ? 1 : 0;
    }
    return idx;
}

// rs_eval.hip -- the lock-step of the Monte-Carlo evaluation of feed-forward agents and teams (algos/multiagent/evaluate.py:355-475;
// radiation_ppo_amd/evaluate.py: run_test_environments_team) as two launches around rs_action_uniforms and rs_step.
//
// rs_ff_eval_step: the policy round.  rs_ff_team_step_kernel's grid, staging, forward pass and sampler (grid = (sample groups, agent),
// a one-wave workgroup stages ITS agent's actor into LDS and serves 64-sample groups of that agent, lane = lane of the evaluation),
// without the critic -- an evaluation throws the value away -- so 21.8 KB of LDS where the step round needs 42.3 KB.  The reading
// (element 0 of a row) is standardised on the way in with rs_welford_standardize_kernel's expression, and the action row of a lane
// whose episode has ended is 8 (idle): no standardised copy of the observation and no masking pass exist.
//
// rs_eval_post_step: everything between rs_step and the next policy round, one thread per lane: return and length, the any-agent
// terminal rule, the Welford update of rs_welford_update_kernel on the lanes still running, the new current observation, and a
// monotonic count of finished lanes that the host reads once every few lock-steps instead of reducing `alive` every step.
//
// The float64 arithmetic is the reference's, operation by operation (the build disables FMA contraction): the results equal
// DeviceWelford's and the torch composition's bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_mlp.hpp"

namespace {

// every agent's actor pointers travel in the kernel's argument block (8 agents x 6 pointers = 384 bytes)
struct RsEvalNets {
    RsMlpParams actor[RS_MAX_AGENTS];
};

// amdgpu_waves_per_eu(2): as rs_ff_team_step_kernel -- a second one-wave workgroup on the SIMD hides this one's weight fill
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
rs_ff_eval_step_kernel(RsEvalNets nets, int A, const float* __restrict__ obs, const double* __restrict__ w_mean,
                       const double* __restrict__ w_std, const float* __restrict__ u, const uint8_t* __restrict__ alive,
                       int8_t* __restrict__ act8, int N) {
    extern __shared__ __align__(16) float smem_f[];
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.y;
    const int groups = (N + 63) / 64;
    RsMlpLds<8> Act;
    Act.carve(smem_f);
    Act.fill(nets.actor[a]);
    __syncthreads();
    for (int gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const int n = gi * 64 + lane;
        const bool live = n < N;
        const int nn = live ? n : N - 1;
        const size_t i = (size_t)nn * A + a;
        const float* row = obs + i * RS_IN;
        float xo[RS_IN_PAD], xp[RS_IN_PAD];
#pragma unroll
        for (int k = 0; k < RS_IN; ++k) xo[k] = row[k];
        if (w_mean) xo[0] = (float)(((double)xo[0] - w_mean[i]) / w_std[i]);
        xo[11] = 0.0f;
#pragma unroll
        for (int k = 0; k < RS_IN_PAD; ++k) xp[k] = __shfl_xor(xo[k], 32);
        float lg[8];
        rs_mlp_forward<8>(Act, xo, xp, lg);
        // K6's own-lane sampler (rs_rollout16.hpp): lg - max - log sum exp, running CDF of exp(lp), a = #{j < 7 : cdf_j <= u}
        float mx = lg[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) mx = fmaxf(mx, lg[q]);
        float se = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) se += __expf(lg[q] - mx);
        const float lse = __logf(se);
        const float un = u[i];
        int ai = 0;
        float cdf = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float lpq = (lg[q] - mx) - lse;
            cdf += __expf(lpq);
            if (q < 7) ai += (cdf <= un) ? 1 : 0;
        }
        if (live) act8[i] = alive[nn] != 0 ? (int8_t)ai : (int8_t)8;      // finished episodes idle in place
    }
}

__global__ void __launch_bounds__(256) rs_eval_post_step_kernel(rs_eval_state s) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int A = s.A;
    bool stopped = false;
    if (n < s.N) {
        const float r = s.use_team_reward ? s.env_team[n] : s.env_reward[(size_t)n * A];
        bool alive = s.alive[n] != 0;
        if (alive) {
            s.ep_ret[n] += r;
            s.ep_len[n] += 1;
        }
        bool any = false;
        for (int a = 0; a < A; ++a) any = any || s.env_done[(size_t)n * A + a] != 0;
        const bool found = alive && any;
        if (found) {
            s.success[n] = 1;
            s.alive[n] = 0;
            alive = false;
            stopped = true;
        }
        for (int a = 0; a < A; ++a) {
            const size_t i = (size_t)n * A + a;
            const float* src = s.env_obs + i * RS_OBS_DIM;
            float* dst = s.cur_obs + i * RS_OBS_DIM;
            if (alive && s.w_count) {
                // rs_welford_update_kernel, expression by expression
                const double x = (double)src[0];
                const double c = s.w_count[i] + 1.0, m = s.w_mean[i];
                s.w_count[i] = c;
                if (c == 1.0) {
                    s.w_mean[i] = x;
                } else {
                    const double mn = m + (x - m) / c;
                    const double q = s.w_sq[i] + (x - m) * (x - mn);
                    s.w_mean[i] = mn;
                    s.w_sq[i] = q;
                    s.w_std[i] = fmax(sqrt(q / fmax(c - 1.0, 1.0)), 1.0);
                }
            }
#pragma unroll
            for (int k = 0; k < RS_OBS_DIM; ++k) dst[k] = src[k];
        }
    }
    // one ballot per wave, one atomic by one of its lanes (every lane of the wave is here: nothing returned early)
    const unsigned long long b = __ballot(stopped);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(s.finished, (int)__popcll(b));
}

}  // namespace

extern "C" {

int rs_ff_eval_step(const rs_mlp_params* actors, int32_t num_agents, const float* obs, const double* w_mean, const double* w_std,
                    const float* u, const uint8_t* alive, int8_t* act8, int32_t num_envs, rs_stream_t stream) {
    if (!actors || !obs || !u || !alive || !act8 || (w_mean == nullptr) != (w_std == nullptr) || num_agents < 1 ||
        num_agents > RS_MAX_AGENTS || num_envs < 1)
        return RS_ERR_INVALID_ARG;
    RsEvalNets nets;
    for (int a = 0; a < RS_MAX_AGENTS; ++a) {
        const int s = a < num_agents ? a : 0;                      // the slots behind the team repeat agent 0 (never read)
        nets.actor[a] = RsMlpParams{actors[s].w1, actors[s].b1, actors[s].w2, actors[s].b2, actors[s].w3, actors[s].b3};
    }
    const int groups = (num_envs + 63) / 64;
    const int gx = groups < 2048 ? groups : 2048;
    const size_t lds = sizeof(float) * (size_t)rs_mlp_lds_floats(8);
    hipLaunchKernelGGL(rs_ff_eval_step_kernel, dim3(gx, num_agents), dim3(64), lds, static_cast<hipStream_t>(stream), nets, (int)num_agents, obs,
                       w_mean, w_std, u, alive, act8, (int)num_envs);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_eval_post_step(const rs_eval_state* s, rs_stream_t stream) {
    if (!s || s->N < 1 || s->A < 1 || s->A > RS_MAX_AGENTS || !s->env_obs || !s->env_reward || !s->env_team || !s->env_done || !s->cur_obs || !s->alive ||
        !s->success || !s->ep_len || !s->ep_ret || !s->finished ||
        (s->w_count != nullptr) != (s->w_mean != nullptr) || (s->w_count != nullptr) != (s->w_sq != nullptr) ||
        (s->w_count != nullptr) != (s->w_std != nullptr))
        return RS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rs_eval_post_step_kernel, dim3((s->N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), *s);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

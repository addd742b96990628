// rs_eval.hip -- the lock-step of the Monte-Carlo evaluation of feed-forward agents and teams (algos/multiagent/evaluate.py:355-475;
// radiation_ppo_amd/evaluate.py: run_test_environments_team) as two launches around rs_action_uniforms and rs_step.
//
// rs_ff_eval_step: the policy round.  rs_ff_team_step_kernel's grid, staging, forward pass and sampler (grid = (sample groups, agent),
// a one-wave workgroup stages ITS agent's actor into LDS and serves 64-sample groups of that agent, lane = lane of the evaluation),
// without the critic -- an evaluation throws the value away -- so 21.8 KB of LDS where the step round needs 42.3 KB.  The reading
// (element 0 of a row) is standardised on the way in (rs_welford.hpp), and the action row of a lane
// whose episode has ended is 8 (idle): no standardised copy of the observation and no masking pass exist.
//
// rs_eval_post_step: everything between rs_step and the next policy round, one thread per lane: return and length, the any-agent
// terminal rule, the Welford update (rs_welford.hpp) on the lanes still running, the new current observation, and a
// monotonic count of finished lanes that the host reads once every few lock-steps instead of reducing `alive` every step.
//
// rs_rnn_team_eval_post_step / rs_rnn_team_eval_post_refresh: the same place in the lock-step of RAD-A2C, a team of A >= 1 recurrent
// agents per lane (radiation_ppo_amd/evaluate.py: run_test_environments_rnn_team), where a lane works through `runs_per_lane`
// consecutive runs with its hidden states carried (evaluate.py:353, :455-470): agent 0's return, step counts, the per-run records under
// the any-agent terminal rule, every agent's Welford update and restart, the next observation raw and standardised, the predictor
// bank's call counter and the finished-lane count, one thread per lane.  The team's policy round, rs_rnn_team_eval_step, lives beside
// K14 in rs_rnn_policy.hip.
//
// rs_rnn_eval_post_step / rs_rnn_eval_post_refresh: the A = 1 case under its own struct (no field A); the host widens the struct and
// launches the team kernels.
//
// The float64 arithmetic is the reference's, operation by operation (the build disables FMA contraction): the results equal
// DeviceWelford's and the torch composition's bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_mlp.hpp"
#include "rs_welford.hpp"

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
        if (w_mean) xo[0] = rs_welford_standardized(w_mean, w_std, i, xo[0]);
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
            if (alive && s.w_count) rs_welford_push(s.w_count, s.w_mean, s.w_sq, s.w_std, i, (double)src[0]);
#pragma unroll
            for (int k = 0; k < RS_OBS_DIM; ++k) dst[k] = src[k];
        }
    }
    // one ballot per wave, one atomic by one of its lanes (every lane of the wave is here: nothing returned early)
    const unsigned long long b = __ballot(stopped);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(s.finished, (int)__popcll(b));
}

// ---- RAD-A2C (A recurrent agents per lane, `runs_per_lane` consecutive runs): the state machine between rs_step and the next PFGRU /
// policy round, with every agent's own statistics and rows, the any-agent terminal rule and agent 0's reward (evaluate.py:395-397,
// :411-423, :441-444).  The one-agent exports launch these kernels with A = 1.
// cur_obs <- env_obs and x <- its form with the reading standardised by the (lane, agent)'s statistics
__device__ __forceinline__ void rte_rows(const rs_rnn_team_eval_state& s, size_t i) {
    const float* src = s.env_obs + i * RS_OBS_DIM;
    float* cur = s.cur_obs + i * RS_OBS_DIM;
    float* x = s.x + i * RS_OBS_DIM;
#pragma unroll
    for (int k = 0; k < RS_OBS_DIM; ++k) cur[k] = src[k];
#pragma unroll
    for (int k = 1; k < RS_OBS_DIM; ++k) x[k] = src[k];
    x[0] = rs_welford_standardized(s.w_mean, s.w_std, i, src[0]);
}

__global__ void __launch_bounds__(256) rs_rnn_team_post_step_kernel(rs_rnn_team_eval_state s) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    bool ended = false;
    if (n < s.N) {
        const int R = s.runs_per_lane, A = s.A;
        const bool a = s.active[n] != 0;
        int run = s.run[n], steps = s.steps[n];
        float ret = s.ret[n];
        if (a) {
            ret += s.env_reward[(size_t)n * A];                         // `episode_return[0]` (evaluate.py:400-447)
            steps += 1;
            if (s.pf_calls) s.pf_calls[n] += 1;                         // one counter per lane serves every owner
        }
        bool any = false;
        for (int g = 0; g < A; ++g) any = any || s.env_done[(size_t)n * A + g] != 0;
        const bool found = a && any;
        const bool over = found || (a && steps == s.steps_per_episode);
        if (a) {                                                        // before the episode-over test (evaluate.py:395-397)
            for (int g = 0; g < A; ++g) {
                const size_t i = (size_t)n * A + g;
                rs_welford_push(s.w_count, s.w_mean, s.w_sq, s.w_std, i, (double)s.env_obs[i * RS_OBS_DIM]);
            }
        }
        if (over) {
            if (run >= 0 && run < R) {                                  // an active lane has run < R; never write past the lane's records
                const size_t slot = (size_t)n * R + run;
                s.rec_len[slot] = steps;
                s.rec_ret[slot] = ret;
                s.rec_suc[slot] = found ? 1 : 0;
            }
            run += 1;
            steps = 0;
            ret = 0.0f;
        }
        s.again[n] = (over && run < R) ? 1 : 0;
        if (over && run == R) {
            s.active[n] = 0;
            if (s.idle_act8) {
                for (int g = 0; g < A; ++g) s.idle_act8[(size_t)n * A + g] = 8;
            }
            ended = true;
        }
        if (a) {
            s.run[n] = run;
            s.steps[n] = steps;
            s.ret[n] = ret;
        }
        for (int g = 0; g < A; ++g) rte_rows(s, (size_t)n * A + g);
    }
    // one ballot per wave, one atomic by one of its lanes (every lane of the wave is here: nothing returned early)
    const unsigned long long b = __ballot(ended);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(s.finished, (int)__popcll(b));
}

// after rs_refresh(mask = again): every agent's statistics of the lanes that begin their next run restart on the refreshed reading
// (evaluate.py:456-466); hidden states are not touched (:353)
__global__ void __launch_bounds__(256) rs_rnn_team_post_refresh_kernel(rs_rnn_team_eval_state s) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= s.N || s.again[n] == 0) return;
    for (int g = 0; g < s.A; ++g) {
        const size_t i = (size_t)n * s.A + g;
        rs_welford_restart(s.w_count, s.w_mean, s.w_sq, s.w_std, i, (double)s.env_obs[i * RS_OBS_DIM]);
        rte_rows(s, i);
    }
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

static bool rnn_team_eval_ok(const rs_rnn_team_eval_state* s) {
    return s && s->N >= 1 && s->A >= 1 && s->A <= RS_MAX_AGENTS && s->runs_per_lane >= 1 && s->steps_per_episode >= 1 && s->env_obs &&
           s->env_reward && s->env_done && s->cur_obs && s->x && s->w_count && s->w_mean && s->w_sq && s->w_std && s->active && s->again &&
           s->run && s->steps && s->ret && s->rec_len && s->rec_ret && s->rec_suc && s->finished;
}

int rs_rnn_team_eval_post_step(const rs_rnn_team_eval_state* s, rs_stream_t stream) {
    if (!rnn_team_eval_ok(s)) return RS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rs_rnn_team_post_step_kernel, dim3((s->N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), *s);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

int rs_rnn_team_eval_post_refresh(const rs_rnn_team_eval_state* s, rs_stream_t stream) {
    if (!rnn_team_eval_ok(s)) return RS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rs_rnn_team_post_refresh_kernel, dim3((s->N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), *s);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

// the one-agent entries: rs_rnn_eval_state is rs_rnn_team_eval_state without A, so the struct is widened to a team of one and takes
// the team entry's refusals and kernels
static rs_rnn_team_eval_state team_of_one(const rs_rnn_eval_state& s) {
    return rs_rnn_team_eval_state{s.N, 1, s.runs_per_lane, s.steps_per_episode, s.env_obs, s.env_reward, s.env_done, s.cur_obs, s.x,
                                  s.w_count, s.w_mean, s.w_sq, s.w_std, s.active, s.again, s.run, s.steps, s.ret, s.rec_len, s.rec_ret,
                                  s.rec_suc, s.pf_calls, s.idle_act8, s.finished};
}

int rs_rnn_eval_post_step(const rs_rnn_eval_state* s, rs_stream_t stream) {
    if (!s) return RS_ERR_INVALID_ARG;
    const rs_rnn_team_eval_state t = team_of_one(*s);
    return rs_rnn_team_eval_post_step(&t, stream);
}

int rs_rnn_eval_post_refresh(const rs_rnn_eval_state* s, rs_stream_t stream) {
    if (!s) return RS_ERR_INVALID_ARG;
    const rs_rnn_team_eval_state t = team_of_one(*s);
    return rs_rnn_team_eval_post_refresh(&t, stream);
}

}  // extern "C"

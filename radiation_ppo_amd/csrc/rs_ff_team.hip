// rs_ff_team.hip -- one round of ac.step for every agent of a feed-forward team (train.py:345-357, :476-480; FF_core.py:95-129):
// the policy launch of ppo.TeamCollector's lock-step, the counterpart of rs_rnn_policy_step_rows for the 2x64 tanh MLP.
//
// grid = (sample groups, agent).  A one-wave workgroup stages ITS agent's networks into LDS (rs_mlp.hpp: actor and critic in the
// step round, 42.3 KB; the critic alone in the bootstrap round, 20.2 KB) and serves 64-sample groups of that agent only, lane =
// env.  The rows are gathered straight from the collector's [N][A][11] layout (stride A * 11 floats): no per-agent copy exists.
// A team does not fit K6's one-launch form: one agent's operands there are rs_mlp16_lds_floats(8) + rs_mlp16_lds_floats(1) =
// 5448 + 4993 floats (41.8 KB), four agents 167 KB against the 160 KB of a workgroup.
//
// The forward pass is rs_mlp_forward (exact-f32 v_mfma_f32_32x32x2_f32, the path behind rs_policy_forward); its arithmetic per
// sample does not depend on the lane or the group the sample sits in, so a run sharded over several collectors stores the same
// bits.  Log-softmax, CDF and draw are K6's own-lane sampler (rs_rollout16.hpp), FFActorCritic.act's rule.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_mlp.hpp"

namespace {

// every agent's parameter pointers travel in the kernel's argument block (8 agents x 12 pointers = 768 bytes): no device-side
// table to allocate, fill or keep alive
struct RsTeamNets {
    RsMlpParams actor[RS_MAX_AGENTS];
    RsMlpParams critic[RS_MAX_AGENTS];
};

// amdgpu_waves_per_eu(2): at most 256 registers, so that a second one-wave workgroup fits the SIMD and hides this one's weight fill
// (left alone the compiler spreads over 228 + 112 registers; under the cap 168, nothing spilled)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
rs_ff_team_step_kernel(RsTeamNets nets, int A, const float* __restrict__ x, const float* __restrict__ u, int64_t* __restrict__ act,
                       float* __restrict__ f, int8_t* __restrict__ act8, const uint8_t* __restrict__ mask, int N) {
    extern __shared__ __align__(16) float smem_f[];
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.y;
    const int groups = (N + 63) / 64;
    const bool step = u != nullptr;
    if (!step && mask) {
        // bootstrap round: a workgroup none of whose groups holds a masked env leaves before it stages anything
        bool any = false;
        for (int gi = blockIdx.x; gi < groups; gi += gridDim.x) {
            const int n = gi * 64 + lane;
            any = any || (n < N && mask[n] != 0);
        }
        if (__ballot(any) == 0ull) return;
    }
    RsMlpLds<8> Act; RsMlpLds<1> Crt;
    if (step) {
        Act.carve(smem_f);
        Crt.carve(smem_f + rs_mlp_lds_floats(8));
        Act.fill(nets.actor[a]);
    } else {
        Act.carve(smem_f);                                        // (unused in this round)
        Crt.carve(smem_f);
    }
    Crt.fill(nets.critic[a]);
    __syncthreads();
    for (int gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const int n = gi * 64 + lane;
        const bool live = n < N;
        const int nn = live ? n : N - 1;
        const bool want = live && (step || !mask || mask[nn] != 0);
        if (!step && __ballot(want) == 0ull) continue;             // a group without a masked env: skipped before its rows are read
        const float* row = x + ((size_t)nn * A + a) * RS_IN;
        float xo[RS_IN_PAD], xp[RS_IN_PAD];
#pragma unroll
        for (int k = 0; k < RS_IN; ++k) xo[k] = row[k];
        xo[11] = 0.0f;
#pragma unroll
        for (int k = 0; k < RS_IN_PAD; ++k) xp[k] = __shfl_xor(xo[k], 32);
        float v[1];
        rs_mlp_forward<1>(Crt, xo, xp, v);
        if (!step) {
            if (want) f[((size_t)a * 3 + 2) * N + n] = v[0];
            continue;
        }
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
        const float un = u[(size_t)nn * A + a];
        int ai = 0;
        float cdf = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float lpq = (lg[q] - mx) - lse;
            cdf += __expf(lpq);
            if (q < 7) ai += (cdf <= un) ? 1 : 0;
        }
        float logp = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) logp = (ai == q) ? ((lg[q] - mx) - lse) : logp;
        if (live) {
            act[(size_t)a * N + n] = (int64_t)ai;
            f[((size_t)a * 3 + 0) * N + n] = logp;
            f[((size_t)a * 3 + 1) * N + n] = v[0];
            if (act8) act8[(size_t)n * A + a] = (int8_t)ai;
        }
    }
}

}  // namespace

extern "C" {

int rs_ff_team_step(const rs_mlp_params* actors, const rs_mlp_params* critics, int32_t num_agents, const float* x, const float* u,
                    int64_t* act, float* logp_val_boot, int8_t* act8, const uint8_t* mask, int32_t num_envs, rs_stream_t stream) {
    if (!actors || !critics || !x || !logp_val_boot || num_agents < 1 || num_agents > RS_MAX_AGENTS || num_envs < 1) return RS_ERR_INVALID_ARG;
    if (u && !act) return RS_ERR_INVALID_ARG;
    RsTeamNets nets;
    for (int a = 0; a < RS_MAX_AGENTS; ++a) {
        const int s = a < num_agents ? a : 0;                      // the slots behind the team repeat agent 0 (never read)
        nets.actor[a] = RsMlpParams{actors[s].w1, actors[s].b1, actors[s].w2, actors[s].b2, actors[s].w3, actors[s].b3};
        nets.critic[a] = RsMlpParams{critics[s].w1, critics[s].b1, critics[s].w2, critics[s].b2, critics[s].w3, critics[s].b3};
    }
    const int groups = (num_envs + 63) / 64;
    const int gx = groups < 2048 ? groups : 2048;
    const size_t lds = sizeof(float) * (size_t)(u ? rs_mlp_lds_floats(8) + rs_mlp_lds_floats(1) : rs_mlp_lds_floats(1));
    hipLaunchKernelGGL(rs_ff_team_step_kernel, dim3(gx, num_agents), dim3(64), lds, static_cast<hipStream_t>(stream), nets, (int)num_agents, x, u,
                       act, logp_val_boot, act8, mask, (int)num_envs);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_ERR_HIP;
}

}  // extern "C"

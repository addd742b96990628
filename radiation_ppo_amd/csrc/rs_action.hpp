// rs_action.hpp -- the libm form of the action draw the policy kernels end with: log-softmax over the logits, a running CDF of exp(lp),
// the action a = #{j < NA - 1 : cdf_j <= u} and the log-probability of a.  A collector, an evaluation and a team round must draw the
// same action from the same uniform, bit for bit (the tests compare the kernels with torch.equal; tests/golden/policy_step_parent.npz
// holds the bits).  The kernels that run this copy are those whose every row of an alternated five-round timing against their own copy
// stayed inside that copy's spread (profiles/policy_pieces_timing.txt): rs_cnn_head_kernel (rs_cnn_loss.hip) and sk_heads_kernel
// (rs_cnn_eval.hip).  The others keep the same text written out, with the reason beside them;
// the two must be kept in step by hand.  (The __expf form of rs_ff_team.hip, rs_eval.hip and K6 has not been timed on a shared copy
// and stays written out in each.)  The operation order is part of the contract: do not reassociate.
#pragma once
#include <hip/hip_runtime.h>

// lg: the logits, the first NA entries are read.  A caller that does not use lp_sel leaves
// it unused and the compiler drops its selects.
template <int NA, int NL>
__device__ __forceinline__ void rs_draw_action(const float (&lg)[NL], float uu, int& act, float& lp_sel) {
    static_assert(NA <= NL, "NA logits are read");
    float mx = lg[0];
#pragma unroll
    for (int o = 1; o < NA; ++o) mx = fmaxf(mx, lg[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < NA; ++o) se += expf(lg[o] - mx);
    const float lse = logf(se);
    float cdf = 0.0f, sel = (lg[0] - mx) - lse;
    int a = 0;
#pragma unroll
    for (int o = 0; o < NA; ++o) {
        const float lp = (lg[o] - mx) - lse;
        cdf += expf(lp);
        if (o < NA - 1 && cdf <= uu) { a = o + 1; }
    }
#pragma unroll
    for (int o = 1; o < NA; ++o) if (a == o) sel = (lg[o] - mx) - lse;
    act = a;                                               // (locals up to here: a conditional store through a reference stays a branch)
    lp_sel = sel;
}

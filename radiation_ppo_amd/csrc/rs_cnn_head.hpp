// rs_cnn_head.hpp -- the RAD-TEAM (CNN) heads behind h1 = ReLU(y1): Linear(32, 16) -> ReLU -> Linear(16, OUT), OUT = 8 with the action
// draw (csrc/rs_action.hpp) or OUT = 1 for the state value.  One image per lane; the weights are wave uniform and come through the
// scalar unit.  Every layer is one fmaf chain behind its bias, in index order.  Run by rs_cnn_head_kernel<8> / <1> (rs_cnn_loss.hip)
// and by sk_heads_kernel (rs_cnn_eval.hip), whose rows of the alternated five-round timing stayed inside their own copies' spread
// (profiles/policy_pieces_timing.txt).  The evaluation heads and rs_cnn_team_step_head_kernel (rs_cnn_eval.hip: eh_finish, ts_hidden,
// ts_draw) keep the same arithmetic written out, with the reason beside them; the two must be kept in step by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radsearch.h"
#include "rs_action.hpp"
#include "rs_sstream.hpp"

constexpr int RS_HEAD_H1 = 32, RS_HEAD_H2 = 16, RS_HEAD_NA = 8;

// Linear(32, 16) -> ReLU on h1 = ReLU(y1)
__device__ __forceinline__ void rs_cnn_head_layer2(const float* w2_, const float* b2_, const float (&h1)[RS_HEAD_H1], float (&h2)[RS_HEAD_H2]) {
    const rs_cmem_t w2 = rs_as_cmem(w2_), b2 = rs_as_cmem(b2_);
#pragma unroll
    for (int o = 0; o < RS_HEAD_H2; ++o) {
        float s = b2[o];
#pragma unroll
        for (int k = 0; k < RS_HEAD_H1; ++k) s = __builtin_fmaf(w2[o * RS_HEAD_H1 + k], h1[k], s);
        h2[o] = fmaxf(s, 0.0f);
    }
}

// Linear(16, OUT): the logits (OUT = 8) or the state value (OUT = 1)
template <int OUT>
__device__ __forceinline__ void rs_cnn_head_layer3(const float* w3_, const float* b3_, const float (&h2)[RS_HEAD_H2], float (&out)[OUT]) {
    const rs_cmem_t w3 = rs_as_cmem(w3_), b3 = rs_as_cmem(b3_);
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float s = b3[o];
#pragma unroll
        for (int k = 0; k < RS_HEAD_H2; ++k) s = __builtin_fmaf(w3[o * RS_HEAD_H2 + k], h2[k], s);
        out[o] = s;
    }
}

// Linear(16, 8) -> log-softmax -> the inverse-CDF draw on uu: the action and its log-probability
__device__ __forceinline__ void rs_cnn_head_draw(const float* w3, const float* b3, const float (&h2)[RS_HEAD_H2], float uu, int& a, float& lp_sel) {
    float lg[RS_HEAD_NA];
    rs_cnn_head_layer3<RS_HEAD_NA>(w3, b3, h2, lg);
    rs_draw_action<RS_HEAD_NA>(lg, uu, a, lp_sel);
}

// Linear(16, 1): the state value
__device__ __forceinline__ float rs_cnn_head_value(const float* w3, const float* b3, const float (&h2)[RS_HEAD_H2]) {
    float v[1];
    rs_cnn_head_layer3<1>(w3, b3, h2, v);
    return v[0];
}

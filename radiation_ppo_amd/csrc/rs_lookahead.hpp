// rs_lookahead.hpp -- the env's look-ahead: RadSearch.FIM_step (rad_search_env.py:1768-1799) for every agent of every env and
// all eight moves at once, with a measurement at each candidate position.  Nothing in the env is written.
//
// FIM_step calls take_action (:876-946) with proposed_coordinates = [] -- no collision rule, the rule of rs_step's single-int form
// 16 + a -- reads the candidate detector position and puts the detector back.  The gradient-search controller
// (algos/test_environment/eval/core.py:622-653) looks ahead with a full env step per move instead, which also takes a measurement
// at the candidate; the lane function below gives both.
//
// One lane per (env n, agent a, move k): lane = 8 * pair + k with pair = n * A + a, so a wave holds eight (env, agent) pairs and the
// eight candidates of a pair sit in eight neighbouring lanes.  With obstacles every move needs a shortest path and an intersection
// test; a lane runs the one-lane forms (CN = 1) of rs_shortest_path and rs_is_intersect for its own candidate, so the eight moves of a
// pair are the parallel dimension the env step does not have.  The obstacle layout of a pair's env is staged in LDS by the pair's
// eight lanes (word (o*4+c) of pair slot s at r[(o*4+c)*8 + s]: the lanes of a pair read one word -- a broadcast --, the eight pairs
// consecutive banks).  rs_load_geo is the loader of the lane = env kernels (it places a layout by the env's lane of a 64-env wave
// and finds a shared layout from blockIdx) and does not fit this mapping; rs_peek_load_geo follows rs_step4_kernel's loader.
//
// For a candidate:
//   start   = from_xy[n][a] if given, else the agent's lattice position (state fields x, y)
//   tent    = start + get_step(k)                                                     (:205-224)
//   blocked = enforced boundaries and tent outside the bbox by take_action's test     (:917-925), or in_obstruction(tent) (:935-937)
//             (without enforced boundaries take_action only counts an out-of-bounds START and does not roll back: nothing to do here)
//   xy      = blocked ? start : tent,  moved = !blocked
//   rate at xy, computed fresh exactly as agent_step computes it for an agent that has moved (:486-512): shortest path from the
//             source, Euclidean distance, is_intersect; lam = bkg if intersected, else I / r + bkg (I / r^2 + bkg under
//             falloff = inverse_square); r == 0 is taken as 1 and NO error bit is set (a look-ahead changes nothing)
//   meas    = Poisson(lam) from the serial sampler rs_poisson: key (seed, global env id), counter (candidate index of the sampler's
//             loop, step index of the NEXT rs_step, episode, RS_STREAM_PEEK + 8 a + k) -- the step and episode words
//             rs_action_uniforms uses.
// The rate and the draw are computed for an unmoved candidate too, at its start (an env step of a blocked agent would reuse the
// stale sp_dist instead, :528-567); the gradient-search controller ignores them (its gradient of a blocked move is 0).
#pragma once
#include "rs_device.hpp"

#define RS_PEEK_MOVES 8
#define RS_PEEK_PAIRS (RS_WAVE / RS_PEEK_MOVES)          // (env, agent) pairs of a wave

struct RsPeek {
    int x, y;
    bool moved;
    double lam;
    int64_t meas;
};

// the layout of the env of this lane's pair into the pair's LDS column, by the pair's eight lanes; the caller synchronises
__device__ __forceinline__ void rs_peek_load_geo(const RsParams& P, int n, bool active, int* lds_geo, RsGeo& g) {
    const int lane = threadIdx.x & 63, slot = lane >> 3, k = lane & 7;
    const int gi = active ? n / P.group : 0;
    int no = active ? P.num_obs[gi] : 0;
    for (int w = k; w < 4 * no; w += RS_PEEK_MOVES) lds_geo[w * RS_PEEK_PAIRS + slot] = P.rect[(size_t)w * P.G + gi];
    if (P.uniform_nobs > 0 && active) no = P.uniform_nobs;   // a fixed obstruction_count is wave-uniform (see rs_load_geo)
    g.r = lds_geo; g.stride = RS_PEEK_PAIRS; g.off = slot; g.n = no;
}

// The candidate position of move k (0..7) from (x, y) alone -- what the RID-FIM controller needs of the look-ahead (rs_bpf.hip) --:
// true where the move takes place.
template <bool HAS_OBS>
__device__ __forceinline__ bool rs_lookahead_xy(const RsParams& P, const RsGeo& g, int k, int x, int y, int& cx, int& cy) {
    int dx, dy; rs_action_step(k, dx, dy);
    const int tx = x + dx, ty = y + dy;
    bool blocked = false;
    if (P.enforce) blocked = (tx < P.bx0 || ty < P.by0) || (P.bx1 <= tx || P.by1 <= ty);
    if (HAS_OBS && g.n > 0 && rs_in_obstruction(g, tx, ty)) blocked = true;
    cx = blocked ? x : tx; cy = blocked ? y : ty;
    return !blocked;
}

// The look-ahead of env n, agent a, move k (0..7) from (x, y).  Reads the env's state, writes nothing.
template <bool HAS_OBS>
__device__ __forceinline__ RsPeek rs_lookahead_lane(const RsParams& P, const RsGeo& g, int n, int a, int k, int x, int y) {
    const int sx = P.src_x[n], sy = P.src_y[n], intensity = P.intensity[n], bkg = P.bkg[n];
    const uint32_t episode = P.episode[n] - 1u, t = P.tstep[n];
    RsPeek r;
    r.moved = rs_lookahead_xy<HAS_OBS>(P, g, k, x, y, r.x, r.y);
    const double euc = rs_dist_i(r.x, r.y, sx, sy);
    const double sp = (HAS_OBS && g.n > 0) ? rs_shortest_path<1>(g, P.dsrc, P.N, n, sx, sy, r.x, r.y, 0) : euc;
    const bool inter = (HAS_OBS && g.n > 0) ? rs_is_intersect<1>(g, r.x, r.y, sx, sy, euc, sp, 0) : false;
    if (inter) r.lam = (double)bkg;
    else {
        double d = euc;
        if (d == 0.0) d = 1.0;
        r.lam = (P.falloff ? ((double)intensity / (d * d)) : ((double)intensity / d)) + (double)bkg;
    }
    r.meas = rs_poisson(r.lam, t, episode, RS_STREAM_PEEK + (uint32_t)(RS_PEEK_MOVES * a + k), P.seed, P.env_id_base + (uint32_t)n);
    return r;
}

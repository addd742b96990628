// rs_device.hpp -- device-side building blocks of the radiation-search env for gfx950 (CDNA4).
//
// One environment per wavefront lane.  All geometry is exact integer-lattice arithmetic (int32/int64);
// distances, Poisson rates and rewards are float64 with FP contraction OFF (-ffp-contract=off) so the
// results are the IEEE values the reference's Python floats produce.
//
// Reference behaviour restated here (paths relative to the reference root,
// gym_rad_search/gym_rad_search/envs/rad_search_env.py): get_step :178-224, take_action :876-946,
// agent_step :460-613, is_intersect :1133-1146, in_obstruction :1148-1170, obstruction_sensors
// :1172-1261, correct_coords :1263-1306, create_obs :948-1011, sample_source_loc_pos :1013-1131.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_tables.hpp"

#define RS_WAVE 64
#define RS_OBS_DIM 11
#define RS_MAX_AGENTS 8
#define RS_MAX_OBS 7
#define RS_MAX_VERT (4 * RS_MAX_OBS)
#define RS_IDLE 8
#define RS_ACT_NONE 9          // internal: the reference's step(None) during reset
#define RS_CORRECT_CAP 4096

#define RS_ENVERR_ZERO_DIST 1u
#define RS_ENVERR_IDLE_STALL 2u
#define RS_ENVERR_CORRECT_CAP 4u
#define RS_ENVERR_BAD_ACTION 8u
#define RS_ENVERR_NO_PATH 16u

#define RS_AF_BLOCKED 1
#define RS_AF_INTERSECT 2
#define RS_AF_OOB 4
#define RS_AF_COLLISION 8

#define RS_STREAM_RESET 0u
#define RS_STREAM_STEP 1u      // + agent id
#define RS_STREAM_ACT 32u      // + agent id
#define RS_STREAM_GEOM 64u
#define RS_STREAM_NOISE 96u    // + agent id: the coordinate noise of the observation
#define RS_STREAM_PEEK 128u    // + 8 * agent id + move: the look-ahead's measurement draws (rs_lookahead.hpp), 128..191
#define RS_STREAM_BPF 192u     // + agent id: the particle filter's draws (rs_bpf.hpp); counter word 0 carries the particle / slot index

// ---------------------------------------------------------------------------------------------
// Kernel parameter block (passed by value as kernarg).  All arrays are SoA, env index fastest, so a
// wave's 64 lanes read/write 64 consecutive elements of every field (coalesced 256-/512-byte rows).
struct RsParams {
    int N, A, G;                       // envs, agents, geometry groups (G = ceil(N / group))
    int obstruction_count, enforce, falloff, group;
    int coord_noise, debug;            // coord_noise (:365, :569-580); DEBUG hard-coded spawn (:387-389, :782-785, :1043-1090)
    int uniform_nobs;                  // > 0: every env holds exactly this many rectangles (fixed obstruction_count and no
                                       // saved layout loaded by rs_refresh yet) -> obstacle loops are wave-uniform
    int bx0, by0, bx1, by1;            // bbox
    int sa_x0, sa_y0, sa_x1, sa_y1;    // search area (rad_search_env.py:393-420)
    int oa_lo, oa_hi;                  // observation_area
    int obs_hi_x, obs_hi_y;            // int(search_area[2] * 0.9): exclusive bound of the obstacle seed
    double max_dist, scale;
    uint32_t seed, env_id_base;
    // per env [N]
    int *src_x, *src_y, *intensity, *bkg, *iter_count;
    uint32_t *episode, *tstep, *err;
    uint8_t *done, *epoch_end;
    // per geometry group
    int* num_obs;                      // [G]
    int* rect;                         // [28][G]
    uint32_t* geom_epoch;              // [G]
    double* dsrc;                      // [28][N] geodesic distance source -> rectangle vertex
    // per agent [A][N]
    int *ax, *ay, *oobc;
    double *sp, *prev;
    uint8_t* aflags;
};

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11).  key = (seed, global env id); counter = (draw, step, episode, stream)
struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ double u53(uint32_t lo, uint32_t hi) {
    uint64_t v = (((uint64_t)hi << 32) | lo) >> 11;
    return (double)v * (1.0 / 9007199254740992.0);
}

// sequential integer draws of one reset (or one geometry resample)
struct RsDrawSeq {
    uint32_t k0, k1, c2, c3, idx;
    __device__ __forceinline__ int integers(int lo, int hi) {
        u32x4 o = philox4x32_10(idx, 0u, c2, c3, k0, k1);
        idx += 1;
        uint64_t x = ((uint64_t)o.y << 32) | o.x;
        return lo + (int)__umul64hi(x, (uint64_t)(uint32_t)(hi - lo));
    }
};

// np_random.normal(scale=5, size=2) (rad_search_env.py:570-574): one Philox block -> two 53-bit uniforms -> Box-Muller in float64.
// A real call (not inlined), like the rare Poisson branches below: the float64 log / sincos library code stays out of the register
// budget of the env kernels, which only reach it with coord_noise set.
struct RsNoise2 { double x, y; };
__device__ __noinline__ RsNoise2 rs_coord_noise(uint32_t t, uint32_t episode, uint32_t agent, uint32_t k0, uint32_t k1) {
    const u32x4 o = philox4x32_10(0u, t, episode, RS_STREAM_NOISE + agent, k0, k1);
    const double u1 = 1.0 - u53(o.x, o.y);               // (0, 1]
    const double u2 = u53(o.z, o.w);
    const double rad = 5.0 * sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    return RsNoise2{rad * cs, rad * sn};
}

// The rare branches of the sampler are real function calls (not inlined): their float64 library code (exp, log, lgamma)
// and constants otherwise sit in the register budget of EVERY env kernel -- the obstacle step kernel spilled 64-bit
// addresses to scratch at 256 VGPRs and paid a scratch round trip in nearly every phase (profiles/r02_env_step_phase_cycles.txt).
__device__ __noinline__ int64_t rs_poisson_small(double lam, uint32_t t, uint32_t episode, uint32_t stream, uint32_t k0, uint32_t k1) {
    double enlam = exp(-lam);
    int64_t x = 0;
    double prod = 1.0;
    for (uint32_t i = 0;; ++i) {
        u32x4 o = philox4x32_10(i, t, episode, stream, k0, k1);
        prod *= u53(o.x, o.y);
        if (prod > enlam) x += 1; else return x;
    }
}
// PTRS slow path (~10 % of the draws).  Hormann's test  log(V) + log(invalpha) - log(a/us^2 + b)  <=
// -lam + k log(lam) - lgamma(k+1)  evaluated with ONE log on the left and, for x = k+1 >= 10, the
// Stirling series of lgamma on the right (truncation error < 1e-12 at x = 10):
//   rhs = k log(lam/x) - log(x)/2 - lam + x - log(2 pi)/2 - (1/(12x) - 1/(360x^3) + 1/(1260x^5) - 1/(1680x^7))
__device__ __noinline__ bool rs_ptrs_slow_accept(double v, double us, double k, double lam, double a, double b) {
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double lhs = log(v * invalpha / (a / (us * us) + b));
    const double x = k + 1.0;
    double rhs;
    if (x >= 10.0) {
        const double xi = 1.0 / x, xi2 = xi * xi;
        const double ser = xi * (0.083333333333333333 - xi2 * (0.0027777777777777778 - xi2 * (0.00079365079365079365 - xi2 * 0.00059523809523809524)));
        rhs = k * log(lam / x) - 0.5 * log(x) - lam + x - 0.91893853320467274 - ser;
    } else {
        rhs = -lam + k * log(lam) - lgamma(x);
    }
    return lhs <= rhs;
}

// Poisson(lam): Hormann PTRS for lam >= 10 (what numpy's Generator.poisson does there), the
// multiplication method below 10.  Uniform pair i of the draw comes from Philox counter word 0 = i.
__device__ __forceinline__ int64_t rs_poisson(double lam, uint32_t t, uint32_t episode, uint32_t stream, uint32_t k0, uint32_t k1) {
    if (lam == 0.0) return 0;
    if (lam < 10.0) return rs_poisson_small(lam, t, episode, stream, k0, k1);
    double slam = sqrt(lam);
    double b = 0.931 + 2.53 * slam;
    double a = -0.059 + 0.02483 * b;
    double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (uint32_t i = 0;; ++i) {
        u32x4 o = philox4x32_10(i, t, episode, stream, k0, k1);
        double u = u53(o.x, o.y) - 0.5;
        double v = u53(o.z, o.w);
        double us = 0.5 - fabs(u);
        if (!(us > 0.0)) continue;
        double k = floor((2.0 * a / us + b) * u + lam + 0.43);
        if (us >= 0.07 && v <= vr) return (int64_t)k;
        if (k < 0.0 || (us < 0.013 && v > us)) continue;
        if (rs_ptrs_slow_accept(v, us, k, lam, a, b)) return (int64_t)k;
    }
}

// ---- the grouped form of the same draw (K6, rs_rollout16.hpp).  Candidate i of a draw is a pure function of (i, t, episode, stream,
// key, lam) and the result is the first candidate that passes, so the candidates may be evaluated side by side.  A lone wave pays
// the instruction stream of a loop trip once however many lanes run it, and the serial loop runs until the slowest env of the wave
// has accepted (2.1 trips on average for 16 envs, each with the slow path); the lanes of an env that would idle evaluate the next
// candidates in the same trip instead.
struct RsPtrs { double a, b, vr; };
__device__ __forceinline__ RsPtrs rs_ptrs_setup(double lam) {
    double slam = sqrt(lam);
    double b = 0.931 + 2.53 * slam;
    double a = -0.059 + 0.02483 * b;
    double vr = 0.9277 - 3.6224 / (b - 2.0);
    return RsPtrs{a, b, vr};
}
// One candidate of rs_poisson's loop, operation for operation: true = accepted with the value k; o = its Philox block.
__device__ __forceinline__ bool rs_ptrs_try(const u32x4& o, double lam, const RsPtrs& c, double& k) {
    double u = u53(o.x, o.y) - 0.5;
    double v = u53(o.z, o.w);
    double us = 0.5 - fabs(u);
    if (!(us > 0.0)) return false;
    k = floor((2.0 * c.a / us + c.b) * u + lam + 0.43);
    if (us >= 0.07 && v <= c.vr) return true;
    if (k < 0.0 || (us < 0.013 && v > us)) return false;
    return rs_ptrs_slow_accept(v, us, k, lam, c.a, c.b);
}
// rs_poisson(lam, t, episode, stream, k0, k1) for the envs of a wave in the layout lane = (j = lane & 15, g = lane >> 4), env slot j
// in its four lanes (j, 0..3).  All 64 lanes call it, the lanes of an env with the same arguments except o: lane (j, g), g >= FIRST,
// passes philox4x32_10(g - FIRST, t, episode, stream, k0, k1), the block of candidate g - FIRST (lanes g < FIRST: anything).
// Every such lane evaluates its candidate completely, the slow test included where the candidate is undecided, the env takes the
// accepted candidate of the lowest index, and every lane of the env returns its value.  An env whose 4 - FIRST candidates were all
// rejected (0.2 % of the draws at FIRST = 1) goes on with the serial loop from index 4 - FIRST.  lam == 0 and lam < 10 take
// rs_poisson's paths.
template <int FIRST>
__device__ __forceinline__ int64_t rs_poisson_group(double lam, const u32x4& o, uint32_t t, uint32_t episode, uint32_t stream, uint32_t k0, uint32_t k1) {
    static_assert(FIRST >= 0 && FIRST < 4, "candidates sit in the lanes g = FIRST..3");
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const bool ptrs = !(lam == 0.0) && !(lam < 10.0);
    const RsPtrs c = rs_ptrs_setup(lam);
    double k = 0.0;
    const bool acc = ptrs && g >= FIRST && rs_ptrs_try(o, lam, c, k);
    const unsigned long long won = __ballot(acc) >> j;          // bit 16 q: candidate q - FIRST of this env passed
    int src = -1;
#pragma unroll
    for (int q = 3; q >= FIRST; --q) src = ((won >> (16 * q)) & 1ull) ? q : src;
    const int64_t first = __shfl((long long)k, j + 16 * (src < 0 ? 0 : src));
    if (lam == 0.0) return 0;
    if (lam < 10.0) return rs_poisson_small(lam, t, episode, stream, k0, k1);
    if (src >= 0) return first;
    for (uint32_t i = 4 - FIRST;; ++i) {
        u32x4 oi = philox4x32_10(i, t, episode, stream, k0, k1);
        if (rs_ptrs_try(oi, lam, c, k)) return (int64_t)k;
    }
}
// How many candidates rs_poisson's PTRS loop consumes for this draw (0 where it does not reach the loop): for the probe
// (rs_poisson_probe) and the diagnostic builds.
__device__ __forceinline__ int rs_poisson_count(double lam, uint32_t t, uint32_t episode, uint32_t stream, uint32_t k0, uint32_t k1) {
    if (lam == 0.0 || lam < 10.0) return 0;
    const RsPtrs c = rs_ptrs_setup(lam);
    double k;
    for (uint32_t i = 0;; ++i) {
        u32x4 oi = philox4x32_10(i, t, episode, stream, k0, k1);
        if (rs_ptrs_try(oi, lam, c, k)) return (int)(i + 1);
    }
}

// round(x, 2) of a Python float (rad_search_env.py:613): correctly rounded, ties-to-even on the EXACT
// binary value.  x = m * 2^e exactly, so x*100 = (100 m) / 2^s is classified with integer arithmetic.
__device__ __forceinline__ double rs_round2(double x) {
    uint64_t bits = (uint64_t)__double_as_longlong(x);
    int ex = (int)((bits >> 52) & 0x7ff);
    if (ex == 0x7ff) return x;
    double sgn = (bits >> 63) ? -1.0 : 1.0;
    if (ex == 0) return sgn * 0.0;
    uint64_t m = (bits & 0xFFFFFFFFFFFFFull) | (1ull << 52);
    int s = 1075 - ex;                 // x = m * 2^-s
    if (s <= 0) return x;              // |x| >= 2^52: already an integer
    if (m >= (1ull << 57)) return x;   // unreachable (m < 2^53)
    uint64_t P = m * 100ull;           // < 2^60
    if (s >= 61) return sgn * 0.0;     // |x*100| < 1/2
    uint64_t q = P >> s;
    uint64_t rem = P & ((1ull << s) - 1ull);
    uint64_t half = 1ull << (s - 1);
    if (rem > half || (rem == half && (q & 1ull))) q += 1;
    if (q < 256ull) return sgn * RS_CENT_TAB[q];           // == (double)q / 100.0, looked up
    return sgn * ((double)q / 100.0);
}

__device__ __forceinline__ bool rs_isclose_abs(double a, double b, double abs_tol) {   // math.isclose, rel_tol 1e-9
    if (a == b) return true;
    if (isinf(a) || isinf(b)) return false;
    double diff = fabs(b - a);
    return (diff <= fabs(1e-9 * b)) || (diff <= fabs(1e-9 * a)) || (diff <= abs_tol);
}

__device__ __forceinline__ double rs_dist_i(int ax, int ay, int bx, int by) {          // dist_p :125-136
    double dx = (double)(ax - bx), dy = (double)(ay - by);
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ void rs_action_step(int a, int& dx, int& dy) {              // get_step :205-224
    // 0:(-100,0) 1:(-71,71) 2:(0,100) 3:(71,71) 4:(100,0) 5:(71,-71) 6:(0,-100) 7:(-71,-71) 8:(0,0)
    const int cx = (a == 8) ? 0 : ((a >= 3 && a <= 5) ? 1 : ((a == 2 || a == 6) ? 0 : -1));
    const int cy = (a == 8) ? 0 : ((a >= 1 && a <= 3) ? 1 : ((a == 0 || a == 4) ? 0 : -1));
    const int sz = (a & 1) ? 71 : 100;
    dx = cx * sz; dy = cy * sz;
}
__device__ __forceinline__ void rs_dir_coeff(int a, int& cx, int& cy) {                // :186-202
    cx = (a >= 3 && a <= 5) ? 1 : ((a == 2 || a == 6) ? 0 : -1);
    cy = (a >= 1 && a <= 3) ? 1 : ((a == 0 || a == 4) ? 0 : -1);
}

// ---------------------------------------------------------------------------------------------
// Obstacle layout staged in LDS.  per-lane layout: word (o*4+c) of lane l at r[(o*4+c)*64 + l]
// (conflict-free: consecutive lanes -> consecutive banks); shared layout (a whole wave uses one
// layout): r[o*4+c], every lane reads the same word (LDS broadcast).
struct RsGeo {
    const int* r;
    int stride, off, n;     // n = number of obstacles
    __device__ __forceinline__ int get(int o, int c) const { return r[(o * 4 + c) * stride + off]; }
    __device__ __forceinline__ void rect(int o, int& x0, int& y0, int& x1, int& y1) const {
        x0 = get(o, 0); y0 = get(o, 1); x1 = get(o, 2); y1 = get(o, 3);
    }
    // vertex order of create_obs (:975-983): (x0,y0) (x0,y1) (x1,y1) (x1,y0)
    __device__ __forceinline__ void vertex(int v, int& vx, int& vy) const {
        int o = v >> 2, c = v & 3;
        vx = get(o, (c >= 2) ? 2 : 0);
        vy = get(o, (c == 1 || c == 2) ? 3 : 1);
    }
};

// all lattice quantities fit int32: |coordinate| <= 16000 (rs_create), so |product| <= 1.03e9 and sums of two < 2^31
__device__ __forceinline__ bool rs_frac_lt(int n1, int d1, int n2, int d2) { return n1 * d2 < n2 * d1; }

// closed segment p-q meets the OPEN interior of [x0,x1]x[y0,y1]?  (exact)
__device__ __forceinline__ bool rs_seg_hits_open_rect(int px, int py, int qx, int qy, int x0, int y0, int x1, int y1) {
    // exact prune: the segment's bounding box does not reach into the open rectangle
    if (max(px, qx) <= x0 || min(px, qx) >= x1 || max(py, qy) <= y0 || min(py, qy) >= y1) return false;
    int dx = qx - px, dy = qy - py;
    int ln = -1, ld = 1, un = 2, ud = 1;      // t in (-1, 2) to start: neutral bounds
    bool has = false;
    if (dx == 0) { if (!(x0 < px && px < x1)) return false; }
    else {
        int a = dx > 0 ? (x0 - px) : (px - x1), b = dx > 0 ? (x1 - px) : (px - x0), d = dx > 0 ? dx : -dx;
        ln = a; ld = d; un = b; ud = d; has = true;
    }
    if (dy == 0) { if (!(y0 < py && py < y1)) return false; }
    else {
        int a = dy > 0 ? (y0 - py) : (py - y1), b = dy > 0 ? (y1 - py) : (py - y0), d = dy > 0 ? dy : -dy;
        if (!has || rs_frac_lt(ln, ld, a, d)) { ln = a; ld = d; }
        if (!has || rs_frac_lt(b, d, un, ud)) { un = b; ud = d; }
        has = true;
    }
    if (!has) return true;                    // degenerate segment strictly inside
    return rs_frac_lt(ln, ld, un, ud) && rs_frac_lt(ln, ld, 1, 1) && rs_frac_lt(0, 1, un, ud);
}

__device__ __forceinline__ int rs_orient(int ax, int ay, int bx, int by, int cx, int cy) {
    const int v = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    return (v > 0) - (v < 0);
}
__device__ __forceinline__ bool rs_on_seg(int ax, int ay, int bx, int by, int cx, int cy) {
    return min(ax, bx) <= cx && cx <= max(ax, bx) && min(ay, by) <= cy && cy <= max(ay, by);
}
// vis.intersect(ls1, ls2, eps) on the lattice: the closed segments share a point
__device__ __forceinline__ bool rs_segs_intersect(int ax, int ay, int bx, int by, int cx, int cy, int dx, int dy) {
    int o1 = rs_orient(ax, ay, bx, by, cx, cy), o2 = rs_orient(ax, ay, bx, by, dx, dy);
    int o3 = rs_orient(cx, cy, dx, dy, ax, ay), o4 = rs_orient(cx, cy, dx, dy, bx, by);
    if (o1 != o2 && o3 != o4) return true;
    if (o1 == 0 && rs_on_seg(ax, ay, bx, by, cx, cy)) return true;
    if (o2 == 0 && rs_on_seg(ax, ay, bx, by, dx, dy)) return true;
    if (o3 == 0 && rs_on_seg(cx, cy, dx, dy, ax, ay)) return true;
    if (o4 == 0 && rs_on_seg(cx, cy, dx, dy, bx, by)) return true;
    return false;
}

// edge e of a rectangle in the reference's line_segs order (:1000-1005)
__device__ __forceinline__ void rs_edge(int e, int x0, int y0, int x1, int y1, int& ax, int& ay, int& bx, int& by) {
    ax = (e < 2) ? x0 : x1; ay = (e < 2) ? y0 : y1;
    bx = (e == 0 || e == 2) ? x0 : x1;
    by = (e == 0 || e == 2) ? y1 : y0;
}

// vis.boundary_distance(Line_Segment(p,q), rect) < 0.001, exact
__device__ __forceinline__ bool rs_seg_rect_close(int px, int py, int qx, int qy, int x0, int y0, int x1, int y1) {
    // exact prune: bounding boxes at least 1 apart => distance >= 1 > 0.001
    if (max(px, qx) < x0 - 1 || min(px, qx) > x1 + 1 || max(py, qy) < y0 - 1 || min(py, qy) > y1 + 1) return false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int ax, ay, bx, by; rs_edge(e, x0, y0, x1, y1, ax, ay, bx, by);
        if (rs_segs_intersect(px, py, qx, qy, ax, ay, bx, by)) return true;
    }
    int dx = qx - px, dy = qy - py;
    const int len2 = dx * dx + dy * dy;
    if (len2 == 0) return false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int cx = (c >= 2) ? x1 : x0, cy = (c == 1 || c == 2) ? y1 : y0;
        const int dot = (cx - px) * dx + (cy - py) * dy;
        if (dot >= 0 && dot <= len2) {
            // distance^2 = cr^2 / len2 < 1e-6.  len2 <= 1.5e7 on this lattice, so only |cr| <= 3 can qualify;
            // testing that first also keeps cr^2 * 1e6 far away from int64 overflow (|cr| reaches 4e6).
            const int cr = (cx - px) * dy - (cy - py) * dx;
            if (cr > -4 && cr < 4 && cr * cr * 1000000 < len2) return true;
        }
    }
    return false;
}

__device__ __forceinline__ double rs_dist_pt_axis_seg(int px, int py, int ax, int ay, int bx, int by) {
    int cx = min(max(px, min(ax, bx)), max(ax, bx));
    int cy = min(max(py, min(ay, by)), max(ay, by));
    return rs_dist_i(px, py, cx, cy);
}

// ---------------------------------------------------------------------------------------------
// Cooperative env step: CN lanes of a wave (lane = slot + 16*cj, cj = 0..CN-1) run the SAME env.  Every lane executes the
// whole step redundantly on identical inputs (so control flow agrees inside the group); only the obstacle loops --
// the vertex loop of the shortest path, the rectangle loops, the eight probe directions -- are split by cj and
// combined with exact, order-independent reductions (min / or / integer sum).  Results are bit-identical to CN = 1.
template <int CN> __device__ __forceinline__ bool rs_grp_any(bool b) {
    if (CN == 1) return b;
    int v = b ? 1 : 0;
    v |= __shfl_xor(v, 16); v |= __shfl_xor(v, 32);
    return v != 0;
}
template <int CN> __device__ __forceinline__ int rs_grp_sum(int v) {
    if (CN == 1) return v;
    v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    return v;
}
template <int CN> __device__ __forceinline__ double rs_grp_min(double v) {
    if (CN == 1) return v;
    v = fmin(v, __shfl_xor(v, 16)); v = fmin(v, __shfl_xor(v, 32));
    return v;
}

__device__ __forceinline__ bool rs_visible(const RsGeo& g, int px, int py, int qx, int qy) {
    for (int o = 0; o < g.n; ++o) {
        int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
        if (rs_seg_hits_open_rect(px, py, qx, qy, x0, y0, x1, y1)) return false;
    }
    return true;
}

// world.shortest_path(source, detector).length() (:491-493): Euclid when visible, else best detour
// through a rectangle vertex whose geodesic distance from the source was cached at reset.
template <int CN>
__device__ __forceinline__ double rs_shortest_path(const RsGeo& g, const double* dsrc, int N, int n,
                                                   int sx, int sy, int px, int py, int cj) {
    if (CN == 1) {
        if (rs_visible(g, sx, sy, px, py)) return rs_dist_i(sx, sy, px, py);
    } else {
        bool hit = false;
        for (int o = cj; o < g.n; o += CN) {
            int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
            hit |= rs_seg_hits_open_rect(sx, sy, px, py, x0, y0, x1, y1);
        }
        if (!rs_grp_any<CN>(hit)) return rs_dist_i(sx, sy, px, py);
    }
    double best = INFINITY;
    if (CN == 1) {
        for (int v = 0; v < 4 * g.n; ++v) {
            double d = dsrc[(size_t)v * N + n];
            if (d < best) {                       // exact prune: d + |v-p| >= d, a vertex at d >= best cannot improve
                int vx, vy; g.vertex(v, vx, vy);
                const double c = d + rs_dist_i(vx, vy, px, py);
                if (c < best && rs_visible(g, vx, vy, px, py)) best = c;     // visibility only for improving candidates
            }
        }
    } else {
        // this lane's vertices: corner cj of every rectangle; the cached geodesics are fetched up front (one latency)
        double dv[RS_MAX_VERT / 4];
#pragma unroll
        for (int o = 0; o < RS_MAX_VERT / 4; ++o) dv[o] = (o < g.n) ? dsrc[(size_t)(4 * o + cj) * N + n] : INFINITY;
#pragma unroll
        for (int o = 0; o < RS_MAX_VERT / 4; ++o) {
            if (o < g.n && dv[o] < best) {
                int vx, vy; g.vertex(4 * o + cj, vx, vy);
                const double c = dv[o] + rs_dist_i(vx, vy, px, py);
                if (c < best && rs_visible(g, vx, vy, px, py)) best = c;
            }
        }
        best = rs_grp_min<CN>(best);
    }
    return best;
}

// is_intersect (:1133-1146) for a detector at (px,py)
template <int CN>
__device__ __forceinline__ bool rs_is_intersect(const RsGeo& g, int px, int py, int sx, int sy, double euc, double sp, int cj) {
    if (CN == 1) {
        for (int o = 0; o < g.n; ++o) {
            int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
            if (rs_seg_rect_close(px, py, sx, sy, x0, y0, x1, y1) && !rs_isclose_abs(sqrt(euc), sp, 0.1)) return true;
        }
        return false;
    }
    if (rs_isclose_abs(sqrt(euc), sp, 0.1)) return false;        // the second operand of the `and` does not depend on the rectangle
    bool close = false;
    for (int o = cj; o < g.n; o += CN) {
        int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
        close |= rs_seg_rect_close(px, py, sx, sy, x0, y0, x1, y1);
    }
    return rs_grp_any<CN>(close);
}

// in_obstruction (:1148-1170): first rectangle that contains the point (closed), then strict test on it
__device__ __forceinline__ bool rs_in_obstruction(const RsGeo& g, int px, int py) {
    for (int o = 0; o < g.n; ++o) {
        int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
        if (x0 <= px && px <= x1 && y0 <= py && py <= y1) return (x0 < px && px < x1 && y0 < py && py < y1);
    }
    return false;
}

__device__ __forceinline__ bool rs_pt_in_closed_eps(double qx, double qy, int x0, int y0, int x1, int y1) {
    double dx = fmax(fmax((double)x0 - qx, 0.0), qx - (double)x1);
    double dy = fmax(fmax((double)y0 - qy, 0.0), qy - (double)y1);
    return sqrt(dx * dx + dy * dy) <= 0.0000001;
}

// correct_coords (:1263-1306): walk the eight probe directions outwards in 0.1 cm steps until one of them touches the
// rectangle; returns the bit mask of the touching directions (0 with *capped when the iteration cap was hit).  Rare (a
// detector in a rectangle corner region): kept out of line for the register budget of the env kernels.
__device__ __noinline__ uint32_t rs_correct_walk(int px, int py, int x0, int y0, int x1, int y1, int* capped) {
    double qx[8], qy[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) { qx[a] = (double)px; qy[a] = (double)py; }
    uint32_t chk = 0;
    int it = 0;
    while (chk == 0) {
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            int cx, cy; rs_dir_coeff(a, cx, cy);
            qx[a] = qx[a] + (double)cx * 0.1;
            qy[a] = qy[a] + (double)cy * 0.1;
            if (rs_pt_in_closed_eps(qx[a], qy[a], x0, y0, x1, y1)) chk |= 1u << a;
        }
        if (++it >= RS_CORRECT_CAP) { *capped = 1; break; }
    }
    return chk;
}

// obstruction_sensors (:1172-1261) + correct_coords (:1263-1306).  Writes the 8 readings (float64
// values rounded once to float32, as the PPO buffer does) to out[0..7] (an LDS row).
template <bool HAS_OBS, int CN = 1>
__device__ __forceinline__ void rs_sensors(const RsParams& P, const RsGeo& g, int px, int py, float* out, uint32_t& err, int cj = 0) {
    uint32_t mine = 0xffu;     // directions whose reading this lane holds (CN > 1: two probe directions per lane)
    double d8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d8[i] = 0.0;
    uint32_t near = 0;         // obstacles whose rectangle a 100 cm probe can reach at all (exact prune)
    if (HAS_OBS) {
        for (int o = 0; o < g.n; ++o) {
            int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
            if (!(px + 100 < x0 || px - 100 > x1 || py + 100 < y0 || py - 100 > y1)) near |= 1u << o;
        }
    }
#if defined(RS_ABL) && RS_ABL == 1
    near = 0;
#endif
    if (HAS_OBS && near != 0) {
        uint64_t cnt = 0;      // obs_idx_ls packed 8 bits per obstacle
        int ones = 0;
        if (CN > 1) mine = 3u << (2 * cj);
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) {
            if (CN > 1 && !(mine >> idx & 1u)) continue;
            int sx_, sy_; rs_action_step(idx, sx_, sy_);
            int qx = px + sx_, qy = py + sy_;
            int inter = 0;
            double dmax = 0.0;
            // visit only the obstacles a probe can reach, in ascending index order (the reference's order);
            // the per-lane trip count is popcount(near) (typically 0-1) instead of the obstacle count
            for (uint32_t rem = near; rem != 0; rem &= rem - 1) {
                const int o = __ffs((int)rem) - 1;
                int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
                // exact prune: the probe's bounding box does not touch the rectangle -> no edge can be hit
                if (max(px, qx) < x0 || min(px, qx) > x1 || max(py, qy) < y0 || min(py, qy) > y1) continue;
                double m = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int ax, ay, bx, by; rs_edge(e, x0, y0, x1, y1, ax, ay, bx, by);
                    if (inter < 2 && rs_segs_intersect(ax, ay, bx, by, px, py, qx, qy)) {
                        double od = rs_dist_pt_axis_seg(px, py, ax, ay, bx, by);
                        double ld = (110.0 - od) / 110.0;
                        m = fmax(m, ld);       // max(seg_dist) with the untouched entries at 0.0
                        inter += 1;
                        cnt += 1ull << (8 * o);
                    }
                }
                if (inter > 0 && m > dmax) dmax = m;
            }
            d8[idx] = dmax;
            ones += (dmax == 1.0) ? 1 : 0;
        }
        if (CN > 1) {          // integer sums over the group: per-obstacle hit counts stay below 256 (8 probes x 2 edges)
            ones = rs_grp_sum<CN>(ones);
            const int lo = rs_grp_sum<CN>((int)(uint32_t)cnt), hi = rs_grp_sum<CN>((int)(uint32_t)(cnt >> 32));
            cnt = (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32);
        }
        if (ones > 3) {
            mine = 0xffu;      // every lane recomputes all eight readings from the same inputs
            // argmax = max(zip(obs_idx_ls, self.poly))[1]: count, then vertex list lexicographically
            int best = 0;
            for (int k = 1; k < g.n; ++k) {
                int ck = (int)((cnt >> (8 * k)) & 0xff), cb = (int)((cnt >> (8 * best)) & 0xff);
                bool gt;
                if (ck != cb) gt = ck > cb;
                else {
                    int a0 = g.get(k, 0), a1 = g.get(k, 1), a2 = g.get(k, 2), a3 = g.get(k, 3);
                    int b0 = g.get(best, 0), b1 = g.get(best, 1), b2 = g.get(best, 2), b3 = g.get(best, 3);
                    // key (x0,y0,x0,y1,x1,y1,x1,y0) -> distinct components in order x0,y0,y1,x1
                    if (a0 != b0) gt = a0 > b0; else if (a1 != b1) gt = a1 > b1;
                    else if (a3 != b3) gt = a3 > b3; else gt = a2 > b2;
                }
                if (gt) best = k;
            }
            int x0, y0, x1, y1; g.rect(best, x0, y0, x1, y1);
            int capped = 0;
            const uint32_t chk = rs_correct_walk(px, py, x0, y0, x1, y1, &capped);
            if (capped) err |= RS_ENVERR_CORRECT_CAP;
#pragma unroll
            for (int i = 0; i < 8; ++i) d8[i] = 0.0;
            if (__popc(chk) >= 4) {
#pragma unroll
                for (int ii = 0; ii < 8; ii += 2) {
                    int lo = (ii + 7) & 7, hi = (ii + 1) & 7;
                    if ((chk >> lo & 1u) && (chk >> hi & 1u)) { d8[ii] = 1.0; d8[lo] = 1.0; d8[hi] = 1.0; }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (CN == 1 || (mine >> i & 1u)) out[i] = (float)d8[i];
    if (P.enforce) {
        // walls (:1232-1259): (DIST_TH - |x - wall|) / DIST_TH with an integer distance 0..110 -> exact table
        const int dl = abs(px - P.bx0), dd = abs(py - P.by0), dr = abs(P.bx1 - px), du = abs(P.by1 - py);
        if (px - 110 < P.bx0) out[0] = (dl <= 110) ? RS_WALL_TAB[dl] : (float)((110.0 - (double)dl) / 110.0);
        if (py - 110 < P.by0) out[6] = (dd <= 110) ? RS_WALL_TAB[dd] : (float)((110.0 - (double)dd) / 110.0);
        if (P.bx1 <= px + 110) out[4] = (dr <= 110) ? RS_WALL_TAB[dr] : (float)((110.0 - (double)dr) / 110.0);
        if (P.by1 <= py + 110) out[2] = (du <= 110) ? RS_WALL_TAB[du] : (float)((110.0 - (double)du) / 110.0);
    }
}

// ---------------------------------------------------------------------------------------------
// Outputs of one env (lane) for one lock-step.  obs rows go to an LDS tile (coalesced copy-out by the
// caller); the scalar outputs go straight to HBM.
struct RsOut {
    float* obs_row;        // LDS: this lane's [A][11] rows, row stride RS_OBS_DIM
    float* reward;         // [N,A] or null
    float* team;           // [N] or null
    uint8_t* done;         // [N,A] or null
    uint8_t* oob;          // [N,A] or null
    int32_t* oobc;         // [N,A] or null
    uint8_t* blocked;      // [N,A] or null
    uint8_t* collision;    // [N,A] or null
};

// RadSearch.step for env n (one lane).  act_of(a) returns agent a's action (0..8) or RS_ACT_NONE.
// Mirrors step :443-728 / agent_step :460-613; agents are processed in id order because `done`, the
// team reward and the collision rule are order dependent.
// Diagnostic build only (-DRS_STEP_STAMPS, scripts/step_stamps.py): wave-level s_memtime stamps at the phase boundaries of the
// env step, added to a table nothing else reads.  The product build contains none of it.
#ifdef RS_STEP_STAMPS
static __device__ unsigned long long rs_step_stamp_table[16];
__device__ __forceinline__ unsigned long long rs_es_now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#define RS_ESTAMP_DECL unsigned long long es_last = rs_es_now();
#define RS_ESTAMP(i) do { const unsigned long long t_ = rs_es_now(); \
                          if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) atomicAdd(&rs_step_stamp_table[i], t_ - es_last); \
                          es_last = rs_es_now(); } while (0)
#else
#define RS_ESTAMP_DECL
#define RS_ESTAMP(i) do {} while (0)
#endif

// The state one lock-step reads and writes, as values: what the env arrays hold for env n (RsEnvRegs) and for one of its agents
// (RsAgentRegs).  rs_env_step_lane loads them, runs the core and stores them; K6 (rs_rollout16.hpp, single agent) keeps them in
// registers from one lock-step to the next and touches the arrays only around a reset and at the end of the launch.
struct RsEnvRegs {
    int sx, sy, intensity, bkg, iter_count;
    uint32_t episode, tstep, err;      // episode: the id the draws of this episode are keyed by (the array holds the NEXT id); err: flags not yet OR-ed into P.err
    bool done;
    __device__ __forceinline__ void load(const RsParams& P, int n) {
        sx = P.src_x[n]; sy = P.src_y[n];
        intensity = P.intensity[n]; bkg = P.bkg[n];
        iter_count = P.iter_count[n];
        episode = P.episode[n] - 1u; tstep = P.tstep[n];
        err = 0;
        done = P.done[n] != 0;
    }
    // what a step changes (the per-episode constants are written by the reset alone)
    __device__ __forceinline__ void store(const RsParams& P, int n) {
        P.done[n] = done ? 1 : 0;
        P.iter_count[n] = iter_count;
        P.tstep[n] = tstep;
        if (err) P.err[n] |= err;
        err = 0;
    }
    // every lane takes the copy lane src of its wave holds
    __device__ __forceinline__ void from_lane(int src) {
        sx = __shfl(sx, src); sy = __shfl(sy, src); intensity = __shfl(intensity, src); bkg = __shfl(bkg, src);
        iter_count = __shfl(iter_count, src); episode = __shfl(episode, src); tstep = __shfl(tstep, src); err = __shfl(err, src);
        done = __shfl((int)done, src) != 0;
    }
};
struct RsAgentRegs {
    int x, y, oobc;
    double sp, prev;
    uint8_t fl;
    __device__ __forceinline__ void load(const RsParams& P, size_t ia) {
        x = P.ax[ia]; y = P.ay[ia]; sp = P.sp[ia]; prev = P.prev[ia]; oobc = P.oobc[ia]; fl = P.aflags[ia];
    }
    __device__ __forceinline__ void store(const RsParams& P, size_t ia) const {
        P.ax[ia] = x; P.ay[ia] = y; P.sp[ia] = sp; P.prev[ia] = prev; P.oobc[ia] = oobc; P.aflags[ia] = fl;
    }
    __device__ __forceinline__ void from_lane(int src) {
        x = __shfl(x, src); y = __shfl(y, src); oobc = __shfl(oobc, src); sp = __shfl(sp, src); prev = __shfl(prev, src);
        fl = (uint8_t)__shfl((int)fl, src);
    }
};

#ifdef RS_STEP_STAMPS
#define RS_ESTAMP_PARAM , unsigned long long& es_last
#define RS_ESTAMP_ARG , es_last
#elif defined(RS_K6_STAMPS)
// Diagnostic build only (-DRS_K6_STAMPS, scripts/k6_stamps.py): the measurement draw inside K6's env step.  k6p[0]: its wave
// cycles, summed; k6p[1]: the candidates rs_poisson's loop needs for this lane's draw of this step (the wave's largest is the trips
// of the serial loop; K6 reduces it); k6p[2]: the cycles spent counting, summed, which the script takes out of "env step".  The
// other callers of the step core pass a dummy.
#undef RS_ESTAMP_DECL
#define RS_ESTAMP_DECL unsigned long long k6p[3] = {0, 0, 0};
#define RS_ESTAMP_PARAM , unsigned long long (&k6p)[3]
#define RS_ESTAMP_ARG , k6p
__device__ __forceinline__ unsigned long long rs_k6p_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
__device__ __forceinline__ int rs_k6p_wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
#else
#define RS_ESTAMP_PARAM
#define RS_ESTAMP_ARG
#endif

// Agent a's part of RadSearch.step on values: take_action, distances, measurement, reward, observation row and the lock-step's
// outputs.  E is read (done is also set); S is the agent's state before and after.  No env array is touched.
// CN > 1: the cooperative form (see rs_grp_any): lanes cj = 0..CN-1 of a group call this with the same arguments.
// cand (K6's wave 0, all 64 lanes in the call, a == 0): the lane's candidate block of the measurement draw for rs_poisson_group<1>;
// null: the serial rs_poisson.
template <bool HAS_OBS, int CN = 1>
__device__ __forceinline__ void rs_agent_step_core(const RsParams& P, const RsGeo& g, int n, int a, int act, bool collided, RsEnvRegs& E,
                                                   RsAgentRegs& S, const RsOut& O, double& max_reward, bool& have_max, int cj RS_ESTAMP_PARAM,
                                                   const u32x4* cand = nullptr) {
    const int N = P.N, A = P.A;
    const int sx = E.sx, sy = E.sy, intensity = E.intensity, bkg = E.bkg;
    const uint32_t episode = E.episode, t = E.tstep;
    const uint32_t k0 = P.seed, k1 = P.env_id_base + (uint32_t)n;
    uint32_t err = 0;
    bool done = E.done;
    if (act < 0) act = RS_IDLE;                             // -1 == idle (:620-623)
    if (act > RS_ACT_NONE) { err |= RS_ENVERR_BAD_ACTION; act = RS_IDLE; }
    int x = S.x, y = S.y;
    double sp = S.sp, prev = S.prev;
    int oobc = S.oobc;
    uint8_t fl = S.fl & (RS_AF_BLOCKED | RS_AF_INTERSECT);   // oob/collision reset each step (:479-480)
    bool moved = false;
    int px = x, py = y;                                      // agent.detector after take_action
    // ---- take_action :876-946
    if (act != RS_ACT_NONE) {
        if (collided) {
            fl |= RS_AF_COLLISION;
        } else {
            int dx, dy; rs_action_step(act, dx, dy);
            int tx = x + dx, ty = y + dy;
            bool roll_back = false;
            if (P.enforce) {
                if ((tx < P.bx0 || ty < P.by0) || (P.bx1 <= tx || P.by1 <= ty)) { fl |= RS_AF_OOB; oobc += 1; roll_back = true; }
            } else {
                bool lower_b = x < P.sa_x0 || y < P.sa_y0, upper_b = P.sa_x1 < x || P.sa_y1 < y;
                if (lower_b || upper_b) { fl |= RS_AF_OOB; oobc += 1; }
            }
            if (HAS_OBS && g.n > 0 && rs_in_obstruction(g, tx, ty)) { roll_back = true; fl |= RS_AF_BLOCKED; }
            if (!roll_back) { x = tx; y = ty; px = tx; py = ty; moved = true; }
        }
    }
    RS_ESTAMP(1);                                            // take_action, in_obstruction
    // ---- distances, line of sight, measurement, reward :486-567
    double euc = rs_dist_i(x, y, sx, sy);                   // == the stale euc_dist when stalled (position unchanged)
    double reward;
#if defined(RS_ABL) && RS_ABL == 3
    if (moved) sp = euc;
#else
    if (moved) sp = (HAS_OBS && g.n > 0) ? rs_shortest_path<CN>(g, P.dsrc, N, n, sx, sy, x, y, cj) : euc;
#endif
    if (HAS_OBS && !(sp < INFINITY)) err |= RS_ENVERR_NO_PATH;
    RS_ESTAMP(2);                                            // shortest path
#if defined(RS_ABL) && RS_ABL == 2
    bool inter = false;
#else
    bool inter = (HAS_OBS && g.n > 0) ? rs_is_intersect<CN>(g, px, py, sx, sy, euc, sp, cj) : false;
#endif
    fl = (uint8_t)((fl & ~RS_AF_INTERSECT) | (inter ? RS_AF_INTERSECT : 0));
    RS_ESTAMP(3);                                            // is_intersect
    double lam;
    if (inter) lam = (double)bkg;
    else {
        double r = euc;
        if (r == 0.0) { err |= RS_ENVERR_ZERO_DIST; r = 1.0; }
        lam = (P.falloff ? ((double)intensity / (r * r)) : ((double)intensity / r)) + (double)bkg;
    }
#if defined(RS_K6_STAMPS) && !defined(RS_STEP_STAMPS)
    const unsigned long long k6p_t0 = rs_k6p_now();
#endif
    int64_t meas = cand ? rs_poisson_group<1>(lam, *cand, t, episode, RS_STREAM_STEP + (uint32_t)a, k0, k1)
                        : rs_poisson(lam, t, episode, RS_STREAM_STEP + (uint32_t)a, k0, k1);
#if defined(RS_K6_STAMPS) && !defined(RS_STEP_STAMPS)
    {
        const unsigned long long t1 = rs_k6p_now();
        k6p[0] += t1 - k6p_t0;
        k6p[1] = (unsigned long long)rs_poisson_count(lam, t, episode, RS_STREAM_STEP + (uint32_t)a, k0, k1);
        k6p[2] += rs_k6p_now() - t1;
    }
#endif
    RS_ESTAMP(4);                                            // Poisson measurement
    if (moved) {
        if (sp < 110.0) { reward = 0.1; done = true; }
        else if (sp < prev) { reward = 0.1; prev = sp; }
        else reward = ((act == RS_IDLE) ? -1.0 : -0.5) * sp / P.max_dist;
    } else {
        if (act == RS_IDLE && !(fl & RS_AF_COLLISION)) err |= RS_ENVERR_IDLE_STALL;
        reward = -0.5 * sp / P.max_dist;
    }
    reward = rs_round2(reward);
    // ---- observation :570-593
    float* row = O.obs_row + a * RS_OBS_DIM;
    row[0] = (float)(double)meas;
    double nx = 0.0, ny = 0.0;
    if (P.coord_noise) { const RsNoise2 nz = rs_coord_noise(t, episode, (uint32_t)a, k0, k1); nx = nz.x; ny = nz.y; }
    row[1] = (float)(((double)x + nx) * P.scale);
    row[2] = (float)(((double)y + ny) * P.scale);
    RS_ESTAMP(5);                                            // reward, observation head
    if ((HAS_OBS && g.n > 0) || P.enforce) rs_sensors<HAS_OBS, CN>(P, g, px, py, row + 3, err, cj);
    else {
#pragma unroll
        for (int i = 0; i < 8; ++i) row[3 + i] = 0.0f;
    }
    RS_ESTAMP(6);                                            // obstruction sensors
    // ---- team reward with the falsy-reset quirk :662-665
    if (!have_max || max_reward == 0.0) { max_reward = reward; have_max = true; }
    else if (max_reward < reward) max_reward = reward;
    S.x = x; S.y = y; S.sp = sp; S.prev = prev; S.oobc = oobc; S.fl = fl;
    E.done = done; E.err |= err;
    const size_t oa = (size_t)n * A + a;
    if (O.reward) O.reward[oa] = (float)reward;
    if (O.done) O.done[oa] = done ? 1 : 0;
    if (O.oob) O.oob[oa] = (fl & RS_AF_OOB) ? 1 : 0;
    if (O.oobc) O.oobc[oa] = oobc;
    if (O.blocked) O.blocked[oa] = (fl & RS_AF_BLOCKED) ? 1 : 0;
    if (O.collision) O.collision[oa] = (fl & RS_AF_COLLISION) ? 1 : 0;
}

// CN > 1: the cooperative form (see rs_grp_any): lanes cj = 0..CN-1 of a group call this with the same n, g, actions and O.
// Every lane of the group stores the (identical) results: duplicate addresses inside one store instruction cost nothing,
// and each lane's later loads of the env state are then ordered after its OWN stores, which the language guarantees.
template <bool HAS_OBS, int CN = 1, typename ActFn>
__device__ __forceinline__ void rs_env_step_lane(const RsParams& P, const RsGeo& g, int n, ActFn act_of, const RsOut& O,
                                                 bool no_collision_rule = false, int cj = 0) {
    const int N = P.N, A = P.A;
    RS_ESTAMP_DECL
    RsEnvRegs E;
    E.load(P, n);

    // collision rule (:908-910): an agent stalls when >1 agents propose its tentative cell.  Proposals
    // are functions of the pre-step positions only, so they are evaluated up front.
    uint32_t coll_mask = 0;
    bool any_none = false;
    for (int i = 0; i < A; ++i) any_none |= (act_of(i) == RS_ACT_NONE);
    if (A > 1 && !any_none && !no_collision_rule) {
        for (int i = 0; i < A; ++i) {
            int dxi, dyi; rs_action_step(act_of(i), dxi, dyi);
            int tx = P.ax[(size_t)i * N + n] + dxi, ty = P.ay[(size_t)i * N + n] + dyi;
            int cnt = 0;
            for (int j = 0; j < A; ++j) {
                int dxj, dyj; rs_action_step(act_of(j), dxj, dyj);
                cnt += (P.ax[(size_t)j * N + n] + dxj == tx && P.ay[(size_t)j * N + n] + dyj == ty) ? 1 : 0;
            }
            if (cnt > 1) coll_mask |= 1u << i;
        }
    }

    double max_reward = 0.0;
    bool have_max = false;
    RS_ESTAMP(0);                                            // state loads, collision proposals
    for (int a = 0; a < A; ++a) {
        const size_t ia = (size_t)a * N + n;
        RsAgentRegs S;
        S.load(P, ia);
        rs_agent_step_core<HAS_OBS, CN>(P, g, n, a, act_of(a), (coll_mask >> a & 1u) != 0, E, S, O, max_reward, have_max, cj RS_ESTAMP_ARG);
        S.store(P, ia);
    }
    if (O.team) O.team[n] = (float)max_reward;
    E.iter_count += 1;
    E.tstep += 1;
    E.store(P, n);
    RS_ESTAMP(7);                                            // write back
}

// ------------------------------------------------------------------------------------------------
// LDS carve-up of one wave.  geo: obstacle rectangles (per-lane or shared layout, see RsGeo);
// tile: the wave's [64][A*11] observation rows (+ odd padding -> conflict-free row writes) that are
// copied out as whole 256-byte rows; flags: which lanes produced a row.
struct WaveLds {
    int* geo;       // 28*64 ints
    float* tile;    // 64 * S floats
    int* flags;     // 64 ints
};
__device__ __forceinline__ int rs_tile_stride(int A) { int s = A * RS_OBS_DIM; return s | 1; }

__device__ __forceinline__ void rs_load_geo(const RsParams& P, int n, bool active, int* lds_geo, RsGeo& g) {
    const int lane = threadIdx.x & 63;
    if (P.obstruction_count == 0) { g.r = lds_geo; g.stride = 0; g.off = 0; g.n = 0; return; }
    const bool shared = (P.group % RS_WAVE) == 0;
    if (shared) {
        const int grp = (blockIdx.x * blockDim.x + (threadIdx.x & ~63)) / P.group;   // wave-uniform
        const int gi = min(grp, P.G - 1);
        if (lane < RS_MAX_VERT) lds_geo[lane] = P.rect[(size_t)lane * P.G + gi];
        g.r = lds_geo; g.stride = 1; g.off = 0; g.n = P.num_obs[gi];
    } else {
        const int gi = active ? n / P.group : 0;
        const int no = active ? P.num_obs[gi] : 0;
        for (int w = 0; w < 4 * no; ++w) lds_geo[w * RS_WAVE + lane] = P.rect[(size_t)w * P.G + gi];
        g.r = lds_geo; g.stride = RS_WAVE; g.off = lane; g.n = no;
    }
    // a fixed obstruction_count is wave-uniform (a kernel argument): loops over obstacles become scalar loops
    if (P.uniform_nobs > 0 && active) g.n = P.uniform_nobs;
}

__device__ __forceinline__ void rs_copy_out(const RsParams& P, float* obs, const float* tile, const int* flags, int wave_env0) {
    if (!obs) return;
    const int lane = threadIdx.x & 63;
    const int row = P.A * RS_OBS_DIM, S = rs_tile_stride(P.A);
    const int total = RS_WAVE * row;
    float* dst = obs + (size_t)wave_env0 * row;
    for (int i = lane; i < total; i += RS_WAVE) {
        int l = i / row, k = i - l * row;
        if (flags[l]) dst[i] = tile[l * S + k];
    }
}


// ------------------------------------------------------------------------------------------------
// rectangles' boundaries share a point  <=>  isclose(boundary_distance(poly1, poly2), 0) (:988)
__device__ __forceinline__ bool rs_rects_touch(int ax0, int ay0, int ax1, int ay1, int bx0, int by0, int bx1, int by1) {
    bool overlap = ax0 <= bx1 && bx0 <= ax1 && ay0 <= by1 && by0 <= ay1;
    bool a_in_b = bx0 < ax0 && ax1 < bx1 && by0 < ay0 && ay1 < by1;
    bool b_in_a = ax0 < bx0 && bx1 < ax1 && ay0 < by0 && by1 < ay1;
    return overlap && !a_in_b && !b_in_a;
}

// create_obs (:948-1011) into a per-lane LDS layout (stride 64) -- draws continue the caller's sequence
__device__ __forceinline__ int rs_create_obs(const RsParams& P, RsDrawSeq& seq, int* lds_geo, int stride, int off) {
    int num = P.obstruction_count;
    if (num == -1) num = seq.integers(1, 6);
    int ii = 0;
    while (ii < num) {
        int sx = seq.integers(P.sa_x0, P.obs_hi_x);
        int sy = seq.integers(P.sa_y0, P.obs_hi_y);
        int ex = seq.integers(P.oa_lo, P.oa_hi);
        int ey = seq.integers(P.oa_lo, P.oa_hi);
        bool touch = false;
        for (int kk = 0; kk < ii && !touch; ++kk) {
            int x0 = lds_geo[(kk * 4 + 0) * stride + off], y0 = lds_geo[(kk * 4 + 1) * stride + off];
            int x1 = lds_geo[(kk * 4 + 2) * stride + off], y1 = lds_geo[(kk * 4 + 3) * stride + off];
            touch = rs_rects_touch(x0, y0, x1, y1, sx, sy, sx + ex, sy + ey);
        }
        if (!touch) {
            lds_geo[(ii * 4 + 0) * stride + off] = sx;
            lds_geo[(ii * 4 + 1) * stride + off] = sy;
            lds_geo[(ii * 4 + 2) * stride + off] = sx + ex;
            lds_geo[(ii * 4 + 3) * stride + off] = sy + ey;
            ii += 1;
        }
    }
    return num;
}

// world.is_valid(EPSILON) (:788) for a layout that passed create_obs: the one VisiLibity clause that can fail is
// "a vertex of hole i is in hole k", i.e. a rectangle nested inside another (boundaries are already disjoint).
__device__ __forceinline__ bool rs_layout_valid(const int* lds_geo, int stride, int off, int num) {
    for (int i = 0; i < num; ++i) {
        const int vx = lds_geo[(i * 4 + 0) * stride + off], vy = lds_geo[(i * 4 + 1) * stride + off];
        for (int k = 0; k < num; ++k) {
            if (k == i) continue;
            const int x0 = lds_geo[(k * 4 + 0) * stride + off], y0 = lds_geo[(k * 4 + 1) * stride + off];
            const int x1 = lds_geo[(k * 4 + 2) * stride + off], y1 = lds_geo[(k * 4 + 3) * stride + off];
            if (x0 <= vx && vx <= x1 && y0 <= vy && vy <= y1) return false;
        }
    }
    return true;
}

// Geodesic distance source -> every rectangle vertex (visibility graph relaxation in per-wave LDS scratch), cached
// in P.dsrc for the episode: rs_shortest_path then needs one visibility test per candidate vertex.
template <bool HAS_OBS, int CN = 1>
__device__ __forceinline__ void rs_source_geodesics(const RsParams& P, const RsGeo& g, int n, int srx, int sry,
                                                    uint32_t* lds_adj, double* lds_d, int slot, int cj = 0) {
    // slot: the env's column of the per-wave scratch.  CN > 1: the lanes of the group take the vertices v = cj (mod CN);
    // visibility is symmetric, so a lane tests only the pairs u < v and the rows are completed from the columns.  The
    // relaxation is order independent: fl(d + w) is monotone in d, so any fair sequence of relaxations descends to the
    // same least fixed point (= the minimum over paths of the left-to-right float64 path sums); it runs until no lane of
    // the group changes a distance.
    const int N = P.N;
    const int V = HAS_OBS ? 4 * g.n : 0;
    for (int v = cj; v < V; v += CN) {
        int vx, vy; g.vertex(v, vx, vy);
        lds_d[v * RS_WAVE + slot] = rs_visible(g, srx, sry, vx, vy) ? rs_dist_i(srx, sry, vx, vy) : INFINITY;
        uint32_t m = 0;
        for (int u = 0; u < v; ++u) {
            int ux, uy; g.vertex(u, ux, uy);
            if (rs_visible(g, ux, uy, vx, vy)) m |= 1u << u;
        }
        lds_adj[v * RS_WAVE + slot] = m;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    uint32_t mine[(RS_MAX_VERT + CN - 1) / CN];      // full adjacency rows of this lane's vertices
#pragma unroll
    for (int i = 0; i < (RS_MAX_VERT + CN - 1) / CN; ++i) {
        const int v = cj + i * CN;
        uint32_t m = 0;
        if (v < V) {
            m = lds_adj[v * RS_WAVE + slot];
            for (int u = v + 1; u < V; ++u) m |= ((lds_adj[u * RS_WAVE + slot] >> v) & 1u) << u;
        }
        mine[i] = m;
    }
    bool changed = V > 0;
    while (changed) {
        changed = false;
#pragma unroll
        for (int i = 0; i < (RS_MAX_VERT + CN - 1) / CN; ++i) {
            const int v = cj + i * CN;
            if (v >= V) continue;
            int vx, vy; g.vertex(v, vx, vy);
            const uint32_t m = mine[i];
            double dv = lds_d[v * RS_WAVE + slot];
            for (uint32_t rem = m; rem != 0; rem &= rem - 1) {
                const int u = __ffs((int)rem) - 1;
                int ux, uy; g.vertex(u, ux, uy);
                double c = lds_d[u * RS_WAVE + slot] + rs_dist_i(ux, uy, vx, vy);
                if (c < dv) { dv = c; changed = true; }
            }
            lds_d[v * RS_WAVE + slot] = dv;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        changed = rs_grp_any<CN>(changed);
    }
    for (int v = 0; v < V; ++v) P.dsrc[(size_t)v * N + n] = lds_d[v * RS_WAVE + slot];
}

// ---------------------------------------------------------------------------------------------
// RadSearch.reset for env n (one lane): rad_search_env.py:730-797 with create_obs (per-env layouts),
// sample_source_loc_pos :1013-1131, the source->vertex geodesic cache, and the initial step(None).
// lds_adj / lds_d: per-wave scratch [28][64] (u32 / f64), only touched when HAS_OBS.
// CN > 1: cooperative form (see rs_grp_any): the CN lanes of a group call this together with slot = the env's LDS column;
// draws, rejection loops and stores are replicated (identical in every lane), the geodesic cache and the first step split.
template <bool HAS_OBS, int CN = 1>
__device__ __forceinline__ void rs_env_reset_lane(const RsParams& P, RsGeo& g, int n, int* lds_geo, uint32_t* lds_adj,
                                                  double* lds_d, float* obs_row, const RsOut& O, int slot = -1, int cj = 0) {
    const int lane = (slot >= 0) ? slot : (int)(threadIdx.x & 63);
    const int N = P.N, A = P.A;
    const uint32_t episode = P.episode[n];
    RsDrawSeq seq{P.seed, P.env_id_base + (uint32_t)n, episode, RS_STREAM_RESET, 0u};
    // ---- per-env obstacle layout (geom_group_size == 1): resample when epoch_end is set (:744-762)
    bool resample = false;
    if (HAS_OBS && P.group == 1) {
        g.r = lds_geo; g.stride = RS_WAVE; g.off = lane;
        resample = P.epoch_end[n] != 0;
        if (!resample) {
            g.n = P.num_obs[n];
            for (int w = 0; w < 4 * g.n; ++w) lds_geo[w * RS_WAVE + lane] = P.rect[(size_t)w * P.G + n];
        }
    }
    P.epoch_end[n] = 0;
    // "Environment is not valid, retrying!" (:788-791): a layout that fails world.is_valid costs a complete nested
    // reset -- its source/detector/intensity draws are consumed, then everything is drawn again -- and one more
    // step(None) per rejected layout after the loop.
    int extra_idle = 0;
    int srx, sry, dtx, dty, intensity, bkg;
    for (;;) {
    if (resample) {
        g.n = rs_create_obs(P, seq, lds_geo, RS_WAVE, lane);
    }
    // ---- sample_source_loc_pos (:1013-1131); rand_point uses the x-range for both axes (:1033)
    srx = seq.integers(P.sa_x0, P.sa_x1); sry = seq.integers(P.sa_x0, P.sa_x1);
    if (P.debug) { srx = 500; sry = 500; }              // DEBUG_SOURCE_LOCATION: the draws above are still consumed (:1040-1044)
    dtx = seq.integers(P.sa_x0, P.sa_x1); dty = seq.integers(P.sa_x0, P.sa_x1);
    if (P.debug) { dtx = 1000; dty = 1000; }            // DEBUG_DETECTOR_LOCATION (:1050-1053)
    for (;;) {
        bool inside = false;
        for (int o = 0; o < g.n && !inside; ++o) {
            int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
            inside = (x0 <= dtx && dtx <= x1 && y0 <= dty && dty <= y1);
        }
        if (!inside) break;
        dtx = seq.integers(P.sa_x0, P.sa_x1); dty = seq.integers(P.sa_x0, P.sa_x1);
    }
    int num_retry = 0;
    for (; !P.debug;) {                                 // DEBUG: no minimum-distance / line-of-sight resampling (:1087-1088)
        while (rs_dist_i(dtx, dty, srx, sry) < 1000.0) { srx = seq.integers(P.sa_x0, P.sa_x1); sry = seq.integers(P.sa_x0, P.sa_x1); }
        bool resamp = false, inter = false;
        for (int o = 0; o < g.n && !resamp; ++o) {
            int x0, y0, x1, y1; g.rect(o, x0, y0, x1, y1);
            if (x0 <= srx && srx <= x1 && y0 <= sry && sry <= y1) resamp = true;
            if (!resamp && rs_seg_rect_close(dtx, dty, srx, sry, x0, y0, x1, y1)) inter = true;
        }
        if (g.n == 0 || (num_retry > 20 && !resamp)) break;
        else if (resamp || !inter) { srx = seq.integers(P.sa_x0, P.sa_x1); sry = seq.integers(P.sa_x0, P.sa_x1); num_retry += 1; }
        else break;
    }
    intensity = seq.integers(1000000, 10000000);    // :778
    bkg = seq.integers(10, 51);                     // :779
    if (P.debug) { intensity = 1000000; bkg = 0; }  // :782-785
    if (!resample || rs_layout_valid(lds_geo, RS_WAVE, lane, g.n)) break;
    extra_idle += 1;
    }
    if (resample) {
        P.num_obs[n] = g.n;
        for (int w = 0; w < 4 * g.n; ++w) P.rect[(size_t)w * P.G + n] = lds_geo[w * RS_WAVE + lane];
    }
    rs_source_geodesics<HAS_OBS, CN>(P, g, n, srx, sry, lds_adj, lds_d, lane, cj);
    double prev = (HAS_OBS && g.n > 0) ? rs_shortest_path<CN>(g, P.dsrc, N, n, srx, sry, dtx, dty, cj) : rs_dist_i(srx, sry, dtx, dty);
    // ---- state write (Agent.reset :292-301, reset :736-742, :771-776)
    P.src_x[n] = srx; P.src_y[n] = sry; P.intensity[n] = intensity; P.bkg[n] = bkg;
    P.done[n] = 0; P.iter_count[n] = 0; P.tstep[n] = 0;
    for (int a = 0; a < A; ++a) {
        size_t ia = (size_t)a * N + n;
        P.ax[ia] = dtx; P.ay[ia] = dty; P.sp[ia] = prev; P.prev[ia] = prev; P.oobc[ia] = 0; P.aflags[ia] = 0;
    }
    // ---- initial observation: step(None) (:794-797)
    RsOut o = O;
    o.obs_row = obs_row;
    P.episode[n] = episode + 1;       // draws of this episode are keyed by `episode`
    for (int k = 0; k <= extra_idle; ++k) {
        rs_env_step_lane<HAS_OBS, CN>(P, g, n, [](int) -> int { return RS_ACT_NONE; }, o, false, cj);
        P.iter_count[n] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// RadSearch.refresh_environment for env n (rad_search_env.py:799-874): start an episode from SAVED parameters
// (source, detector start, intensity, background, optionally the obstacle rectangles) instead of sampling them --
// the evaluation harness replays its test-environment sets this way (evaluate.py:346).
// As in the reference, sp_dist is left STALE by this call: its step(None) copies the previous episode's
// prev_det_dist into sp_dist (:562) and only afterwards is prev_det_dist recomputed for the new geometry (:866-868),
// so until the first move that succeeds a stalled step is priced with the old distance.
struct RsRefresh {
    const int32_t* src;        // [N][2]
    const int32_t* det;        // [N][2]
    const int32_t* intensity;  // [N]
    const int32_t* bkg;        // [N]
    const int32_t* num_obs;    // [N] or nullptr: keep the env's current layout (refresh_environment's num_obs = 0 default)
    const int32_t* rects;      // [N][RS_MAX_OBS][4] (x0,y0,x1,y1) when num_obs is given
};

template <bool HAS_OBS>
__device__ __forceinline__ void rs_env_refresh_lane(const RsParams& P, RsGeo& g, int n, const RsRefresh& R, int* lds_geo,
                                                    uint32_t* lds_adj, double* lds_d, float* obs_row, const RsOut& O) {
    const int lane = threadIdx.x & 63;
    const int N = P.N, A = P.A;
    const uint32_t episode = P.episode[n];
    if (HAS_OBS && P.group == 1) {
        g.r = lds_geo; g.stride = RS_WAVE; g.off = lane;
        if (R.num_obs) {
            int num = R.num_obs[n];
            num = num < 0 ? 0 : (num > RS_MAX_OBS ? RS_MAX_OBS : num);
            for (int w = 0; w < 4 * num; ++w) {
                const int v = R.rects[(size_t)n * RS_MAX_OBS * 4 + w];
                lds_geo[w * RS_WAVE + lane] = v;
                P.rect[(size_t)w * P.G + n] = v;
            }
            P.num_obs[n] = num;
            g.n = num;
        } else {
            g.n = P.num_obs[n];
            for (int w = 0; w < 4 * g.n; ++w) lds_geo[w * RS_WAVE + lane] = P.rect[(size_t)w * P.G + n];
        }
    }
    P.epoch_end[n] = 0;                                                   // :810
    const int srx = R.src[2 * n], sry = R.src[2 * n + 1], dtx = R.det[2 * n], dty = R.det[2 * n + 1];
    rs_source_geodesics<HAS_OBS>(P, g, n, srx, sry, lds_adj, lds_d, lane);
    const double prev = (HAS_OBS && g.n > 0) ? rs_shortest_path<1>(g, P.dsrc, N, n, srx, sry, dtx, dty, 0) : rs_dist_i(srx, sry, dtx, dty);
    P.src_x[n] = srx; P.src_y[n] = sry; P.intensity[n] = R.intensity[n]; P.bkg[n] = R.bkg[n];
    P.done[n] = 0; P.iter_count[n] = 0; P.tstep[n] = 0;                   // :811-812
    for (int a = 0; a < A; ++a) {                                         // Agent.reset + det_coords (:823-826)
        size_t ia = (size_t)a * N + n;
        P.ax[ia] = dtx; P.ay[ia] = dty; P.sp[ia] = P.prev[ia]; P.prev[ia] = prev; P.oobc[ia] = 0; P.aflags[ia] = 0;
    }
    RsOut o = O;
    o.obs_row = obs_row;
    P.episode[n] = episode + 1;                                           // a fresh Philox episode, as after reset
    rs_env_step_lane<HAS_OBS>(P, g, n, [](int) -> int { return RS_ACT_NONE; }, o);     // :860
    P.iter_count[n] = 1;                                                  // :870
}

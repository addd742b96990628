// rs_welford.hpp -- the running statistics of a reading (StatisticStandardization, NeuralNetworkCores/RADTEAM_core.py:188-277; StatBuff
// in RADA2C_core.py), the one definition every kernel that keeps or reads them shares.  float64 state, the reference's arithmetic
// operation by operation (the build disables FMA contraction): the results equal DeviceWelford(impl="torch") bit for bit.
//
// Two forms.  The library kernels (rs_welford.hip, rs_eval.hip) work on state the caller owns: four arrays in memory with one stream
// per (env, agent), indexed by i.  K6 (rs_rollout16.hpp) is the benchmark's hot path and holds one env's state in registers for a whole
// rollout: RsWelford.  K6 divides by count - 1, the memory form by fmax(count - 1, 1); the two agree whenever the count is a whole
// number, and each stays as it is so that neither kernel family's instruction stream moves.
//
// The pointers are plain, not __restrict__: a caller's four arrays come out of one struct, and a no-alias promise made here lets the
// compiler reorder the caller's own loads and stores around the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// StatisticStandardization.update (RADTEAM_core.py:215-251) with reading x
__device__ __forceinline__ void rs_welford_push(double* count, double* mean, double* sq, double* sd, size_t i, double x) {
    const double c = count[i] + 1.0, m = mean[i];
    count[i] = c;
    if (c == 1.0) {                                         // first sample: mean = x, sq and std stay (:237-240)
        mean[i] = x;
        return;
    }
    const double mn = m + (x - m) / c;
    const double s = sq[i] + (x - m) * (x - mn);
    mean[i] = mn;
    sq[i] = s;
    sd[i] = fmax(sqrt(s / fmax(c - 1.0, 1.0)), 1.0);
}

// an episode begins with reading x: the reset followed by the first update, which sets the mean only
__device__ __forceinline__ void rs_welford_restart(double* count, double* mean, double* sq, double* sd, size_t i, double x) {
    count[i] = 1.0;
    mean[i] = x;
    sq[i] = 0.0;
    sd[i] = 1.0;
}

// the reading as the networks see it
__device__ __forceinline__ float rs_welford_standardized(const double* mean, const double* sd, size_t i, float reading) {
    return (float)(((double)reading - mean[i]) / sd[i]);
}

// K6: fused collector (rs_rollout16.hpp).  Per-episode Welford standardisation state of one env:
struct RsWelford {
    double count, mean, sq, std;
    __device__ __forceinline__ void update(double x) {          // StatisticStandardization.update (RADTEAM_core.py:215-251)
        count += 1.0;
        if (count == 1.0) { mean = x; }
        else {
            double mean_new = mean + (x - mean) / count;
            sq = sq + (x - mean) * (x - mean_new);
            mean = mean_new;
            std = fmax(sqrt(sq / (count - 1.0)), 1.0);
        }
    }
    __device__ __forceinline__ float standardize(float x) const { return (float)(((double)x - mean) / std); }
    __device__ __forceinline__ void reset() { count = 0.0; mean = 0.0; sq = 0.0; std = 1.0; }
};

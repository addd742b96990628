// mfma4_chain_bits.hip -- is a chain of 32 v_mfma_f32_4x4x1_16b_f32 onto one accumulator, bit for bit, the fmaf chain of the VALU,
// also where products and partial sums are subnormal and where operands are NaN, infinite or -0?  (K7's actor output layer,
// csrc/rs_ppo_grad2.hpp, relies on it.)  Block b of the instruction: D[i][j] = A[lane 4b + i] * B[lane 4b + j] + C, in register i
// of lane 4b + j; the reference lets every lane run the four fmaf chains of its registers.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o mfma4_chain_bits mfma4_chain_bits.hip ; run on the GPU box
// (exit code 0 = every bit agrees in every scenario).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define NS 8
#define K 32
__global__ void k(const float* A, const float* B, unsigned* dm, unsigned* dv) {
    const int l = threadIdx.x;
    for (int s = 0; s < NS; ++s) {
        const float* a = A + s * K * 64;
        const float* b = B + s * K * 64;
        f32x4 m = {0.0f, 0.0f, 0.0f, 0.0f};
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < K; ++q) {
            m = __builtin_amdgcn_mfma_f32_4x4x1f32(a[q * 64 + l], b[q * 64 + l], m, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaf(a[q * 64 + (l & ~3) + i], b[q * 64 + l], v[i]);
        }
        for (int i = 0; i < 4; ++i) {
            dm[(s * 4 + i) * 64 + l] = __float_as_uint(m[i]);
            dv[(s * 4 + i) * 64 + l] = __float_as_uint(v[i]);
        }
    }
}
static unsigned rnd_state = 12345u;
static float rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return (float)((rnd_state >> 8) & 0xffff) / 32768.0f - 1.0f; }   // [-1, 1)
int main() {
    static float hA[NS * K * 64], hB[NS * K * 64];
    static unsigned hm[NS * 4 * 64], hv[NS * 4 * 64];
    const char* names[NS] = {"normal", "A 1e-38 (subnormal products)", "B 1e-38", "A 1e-19, B 1e-19 (sums cross 1.18e-38)", "NaN in B",
                             "NaN in A", "inf in A, some B = 0", "-0 and tiny"};
    for (int s = 0; s < NS; ++s)
        for (int q = 0; q < K; ++q)
            for (int l = 0; l < 64; ++l) {
                float a = 0.25f * rnd(), b = rnd();
                if (s == 1) a *= 4e-38f;
                if (s == 2) b *= 1e-38f;
                if (s == 3) { a *= 4e-19f; b *= 1e-19f; }
                if (s == 4 && q == 7 && (l % 5) == 0) b = NAN;
                if (s == 4 && q == 19 && (l % 7) == 0) b = -NAN;
                if (s == 5 && q == 11 && (l % 3) == 0) a = NAN;
                if (s == 6 && q == 5 && (l % 4) == 1) a = INFINITY;
                if (s == 6 && q == 23 && (l % 4) == 2) a = -INFINITY;
                if (s == 6 && q == 5 && (l % 6) == 0) b = 0.0f;
                if (s == 7) { a = (q & 1) ? -0.0f : a * 1e-30f; b = (l & 1) ? 0.0f : b * 1e-30f; }
                hA[(s * K + q) * 64 + l] = a; hB[(s * K + q) * 64 + l] = b;
            }
    float *A, *B; unsigned *dm, *dv;
    if (hipMalloc(&A, sizeof hA) || hipMalloc(&B, sizeof hB) || hipMalloc(&dm, sizeof hm) || hipMalloc(&dv, sizeof hv)) return 2;
    if (hipMemcpy(A, hA, sizeof hA, hipMemcpyHostToDevice) || hipMemcpy(B, hB, sizeof hB, hipMemcpyHostToDevice)) return 2;
    k<<<1, 64>>>(A, B, dm, dv);
    if (hipMemcpy(hm, dm, sizeof hm, hipMemcpyDeviceToHost) || hipMemcpy(hv, dv, sizeof hv, hipMemcpyDeviceToHost)) return 2;
    int bad_all = 0;
    for (int s = 0; s < NS; ++s) {
        int bad = 0, sub = 0, nan = 0;
        for (int i = 0; i < 4 * 64; ++i) {
            const unsigned m = hm[s * 256 + i], v = hv[s * 256 + i];
            float f; memcpy(&f, &v, 4);
            if (f != 0.0f && fabsf(f) < 1.17549435e-38f) ++sub;
            if (f != f) ++nan;
            if (m != v && bad++ < 4) printf("   scenario %d register %d lane %d: mfma %08x valu %08x\n", s, i / 64, i % 64, m, v);
        }
        printf("%-40s %3d of 256 words differ (%d subnormal results, %d NaN)\n", names[s], bad, sub, nan);
        bad_all += bad;
    }
    return bad_all != 0;
}

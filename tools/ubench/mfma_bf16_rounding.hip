// How does ONE v_mfma_f32_32x32x16_bf16 round on gfx950?  D = C + sum_k A[i][k] B[k][j], 16 exact bf16 x bf16 products per
// output and an fp32 addend.  The forward implicit-GEMM kernels (dvg_amd/csrc/conv_igemm2.hip) chain six of these per
// (16-channel chunk, tap) into one fp32 accumulator, so what a chain of K / 16 x 6 of them costs in accuracy depends on where
// the instruction rounds: once at the end, once per half of K, per block of four products, to nearest or towards zero.
// tests/forward_ref.py: ordered_fp32_ref emulates the kernels' summation with the model this program finds
// (docs/DESIGN_NOTES_forward_tests.md, "The open question").
//
// Every wave multiplies its own random 32 x 16 by 16 x 32 bf16 matrices onto a random fp32 C (second half of the waves: C = 0);
// the host evaluates each of the 1024 outputs per wave exactly (double holds the 17 terms exactly at these magnitudes) and under
// each candidate model and counts bit-for-bit matches.  Also printed: mean and rms of (D - exact) in units of the result's ulp
// (one round-to-nearest: mean 0, rms 0.29; one truncation: |mean| 0.5 towards zero, rms 0.58).
//
//   hipcc -O2 --offload-arch=gfx950 tools/ubench/mfma_bf16_rounding.hip -o build/mfma_bf16_rounding && build/mfma_bf16_rounding
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

constexpr int WAVES = 64;      // 4 per workgroup

// a: [wave][32 rows][16 k], b: [wave][32 columns][16 k] (fp32 values that are exact bf16s), c / d: [wave][32 rows][32 columns]
__global__ __launch_bounds__(256) void k(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                         float* __restrict__ d) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
    if (wave >= WAVES) return;
    auto frag = [&](const float* row) {      // the lane's eight k-values 8 hh .. 8 hh + 7 as bf16 (the upper 16 bits: exact)
        u32x4_t u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned lo = __float_as_uint(row[8 * hh + 2 * e]) >> 16, hi = __float_as_uint(row[8 * hh + 2 * e + 1]) >> 16;
            u[e] = lo | (hi << 16);
        }
        return __builtin_bit_cast(bf16x8_t, u);
    };
    const bf16x8_t fa = frag(a + ((size_t)wave * 32 + l31) * 16), fb = frag(b + ((size_t)wave * 32 + l31) * 16);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = c[((size_t)wave * 32 + 8 * (r >> 2) + 4 * hh + (r & 3)) * 32 + l31];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) d[((size_t)wave * 32 + 8 * (r >> 2) + 4 * hh + (r & 3)) * 32 + l31] = acc[r];
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double uni() {      // [0, 1)
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}
static float bf16_value() {      // a random value with 8 significant bits over seven binades
    float f = (float)((uni() * 4.0 - 2.0) * std::ldexp(1.0, (int)(uni() * 7.0) - 3));
    uint32_t u;
    memcpy(&u, &f, 4);
    u &= 0xffff0000u;
    memcpy(&f, &u, 4);
    return f;
}
static float rne(double x) { return (float)x; }
static float rtz(double x) {
    float f = (float)x;
    if (std::fabs((double)f) > std::fabs(x)) f = std::nextafterf(f, 0.f);
    return f;
}

int main() {
    std::vector<float> a((size_t)WAVES * 32 * 16), b(a.size()), c((size_t)WAVES * 32 * 32), d(c.size());
    for (auto& v : a) v = bf16_value();
    for (auto& v : b) v = bf16_value();
    for (size_t i = 0; i < c.size(); ++i) c[i] = i < c.size() / 2 ? (float)(uni() * 16.0 - 8.0) : 0.f;
    float *da, *db, *dc, *dd;
    CK(hipMalloc(&da, a.size() * 4)); CK(hipMalloc(&db, b.size() * 4)); CK(hipMalloc(&dc, c.size() * 4)); CK(hipMalloc(&dd, d.size() * 4));
    CK(hipMemcpy(da, a.data(), a.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(db, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dd, 0xff, d.size() * 4));
    hipLaunchKernelGGL(k, dim3(WAVES / 4), dim3(256), 0, 0, da, db, dc, dd);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(d.data(), dd, d.size() * 4, hipMemcpyDeviceToHost));

    const char* names[] = {"one rounding to nearest of C + the 16 products",
                           "one rounding towards zero of C + the 16 products",
                           "products summed and rounded to nearest, then added to C (two roundings)",
                           "two halves of K (k 0-7, then 8-15), to nearest after each",
                           "two halves of K (k 8-15, then 0-7), to nearest after each",
                           "two halves of K (k 0-7, then 8-15), towards zero after each",
                           "four blocks of four products, to nearest after each",
                           "four blocks of four products, towards zero after each",
                           "every product added on its own, to nearest",
                           "every product added on its own, towards zero"};
    constexpr int NM = 10;
    for (int half = 0; half < 2; ++half) {
        long match[NM] = {0}, total = 0, off_layout = 0;
        double mean = 0, sq = 0, worst = 0;
        for (int w = half * WAVES / 2; w < (half + 1) * WAVES / 2; ++w)
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    const float* ar = &a[((size_t)w * 32 + i) * 16];
                    const float* bc = &b[((size_t)w * 32 + j) * 16];
                    const double cc = c[((size_t)w * 32 + i) * 32 + j];
                    const float got = d[((size_t)w * 32 + i) * 32 + j];
                    double p[16], blk[4] = {0, 0, 0, 0}, all = 0;
                    for (int kk = 0; kk < 16; ++kk) { p[kk] = (double)ar[kk] * bc[kk]; blk[kk >> 2] += p[kk]; all += p[kk]; }
                    const double exact = cc + all;
                    float m[NM];
                    m[0] = rne(exact);
                    m[1] = rtz(exact);
                    m[2] = rne(cc + (double)rne(all));
                    m[3] = rne((double)rne(cc + blk[0] + blk[1]) + blk[2] + blk[3]);
                    m[4] = rne((double)rne(cc + blk[2] + blk[3]) + blk[0] + blk[1]);
                    m[5] = rtz((double)rtz(cc + blk[0] + blk[1]) + blk[2] + blk[3]);
                    float s6 = (float)cc, s7 = (float)cc, s8 = (float)cc, s9 = (float)cc;
                    for (int q = 0; q < 4; ++q) { s6 = rne((double)s6 + blk[q]); s7 = rtz((double)s7 + blk[q]); }
                    for (int kk = 0; kk < 16; ++kk) { s8 = rne((double)s8 + p[kk]); s9 = rtz((double)s9 + p[kk]); }
                    m[6] = s6; m[7] = s7; m[8] = s8; m[9] = s9;
                    for (int q = 0; q < NM; ++q) match[q] += memcmp(&m[q], &got, 4) == 0;
                    int ex;
                    std::frexp(exact, &ex);
                    const double ulp = std::ldexp(1.0, ex - 24), e = ((double)got - exact) / ulp;
                    const double toward = exact >= 0 ? e : -e;      // > 0: away from zero
                    mean += toward; sq += e * e;
                    if (std::fabs(e) > worst) worst = std::fabs(e);
                    if (!(std::fabs(e) <= 64.0)) ++off_layout;
                    ++total;
                }
        printf("%s: %ld outputs, %ld further than 64 ulp from the exact value (layout check)\n",
               half == 0 ? "random C" : "C = 0", total, off_layout);
        printf("  (D - exact) / ulp: mean %+.3f (positive: away from zero), rms %.3f, worst %.2f\n", mean / total,
               std::sqrt(sq / total), worst);
        for (int q = 0; q < NM; ++q) printf("  %6.2f %% bit-equal: %s\n", 100.0 * match[q] / total, names[q]);
    }
    return 0;
}

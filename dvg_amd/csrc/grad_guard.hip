// Gradient-norm clipping and the skip of a non-finite step, decided ON THE DEVICE (train.py --clip_grad_norm / --skip_nonfinite):
// the iteration is a captured hipGraph, so the host cannot look at a gradient between the backward pass and the Adam steps.
//
//   dvg_grad_sumsq         partials[b] = sum of squares of chunk b of a flat gradient range, fp64
//   dvg_grad_guard_finish  norm = sqrt(sum of the partials); stat = {norm, clip factor, skip, max finite norm}; counters
// dvg_adam_step_guarded, which obeys the verdict, is in backward.hip beside dvg_adam_step.
//
// Arithmetic of the norm.  Every element is converted to fp64 and squared THERE: an fp32 x fp32 product is exact in fp64 (48
// of 53 significand bits, exponents within +-298), so no square overflows or underflows, and the sum of up to 2^25 finite
// squares (< 2^25 x 2^256) cannot overflow either.  "The fp64 sum is not finite" is therefore EXACTLY "some gradient is Inf or
// NaN": squares are >= 0, so Inf never meets -Inf, Inf stays Inf and NaN stays NaN under the additions.
//
// Order.  Workgroup b owns the fixed chunk [b * GG_CHUNK, (b + 1) * GG_CHUNK) - no grid-stride loop, no grid cap: the number of
// partials is a function of n alone (dvg_grad_sumsq_blocks).  A thread adds its 16-byte pieces in index order into four fp64
// sums (one per vector lane), those as (s0 + s1) + (s2 + s3), the 64 lanes of a wave and then the four
// waves through LDS in wave order by block_sum (dvg_common.h).  No atomics: the same input gives the same bits on every launch, rank and resume.
#include "dvg_common.h"

namespace dvg {

constexpr int GG_THREADS = 256;
constexpr int GG_PIECES = 16;                                  // 16-byte loads per thread
constexpr long GG_CHUNK = (long)GG_THREADS * GG_PIECES * 4;    // 16 384 floats per workgroup

__global__ __launch_bounds__(GG_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, long n4,
                                                                 double* __restrict__ partials) {
    __shared__ double red[4];
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    const long base = (long)blockIdx.x * (GG_CHUNK / 4) + threadIdx.x;
    f32x4 v[GG_PIECES];
#pragma unroll
    for (int k = 0; k < GG_PIECES; ++k) {          // all loads in flight before the first is consumed
        const long i = base + (long)k * GG_THREADS;
        v[k] = i < n4 ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k < GG_PIECES; ++k) {
        const double a = (double)v[k][0], b = (double)v[k][1], c = (double)v[k][2], d = (double)v[k][3];
        s0 += a * a;
        s1 += b * b;
        s2 += c * c;
        s3 += d * d;
    }
    const double s = block_sum<GG_THREADS>((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One workgroup.  Thread t adds partials t, t + 256, ... in that order; then the same tree as above.
__global__ __launch_bounds__(GG_THREADS) void grad_guard_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                        double max_norm, int skip_nonfinite,
                                                                        float* __restrict__ stat, int* __restrict__ counters) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += GG_THREADS) s += partials[i];
    const double sum = block_sum<GG_THREADS>(s, red);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sum);
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1.0); a NaN stays a NaN under the clamp
    double scale = 1.0;
    if (max_norm > 0.0) {
        const double c = max_norm / (norm + 1e-6);
        scale = c > 1.0 ? 1.0 : c;
    }
    const bool finite = isfinite(sum);
    const bool skip = skip_nonfinite && !finite;
    stat[0] = (float)norm;
    stat[1] = (float)scale;
    stat[2] = skip ? 1.f : 0.f;
    if (finite && !((float)norm <= stat[3])) stat[3] = (float)norm;
    counters[0] += 1;
    if (!skip && (float)scale < 1.f) counters[1] += 1;
    if (skip) counters[2] += 1;
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_grad_sumsq_blocks(long n) {
    if (n <= 0) return 0;
    const long b = (n + GG_CHUNK - 1) / GG_CHUNK;
    return b > 0x7fffffffL ? 0 : (int)b;
}

extern "C" int dvg_grad_sumsq(const float* g, long n, double* partials, void* stream) {
    DVG_REQUIRE(g && partials, DVG_ERR_NULL, "dvg_grad_sumsq: NULL pointer");
    DVG_REQUIRE(n > 0 && n % 4 == 0 && dvg_grad_sumsq_blocks(n) > 0, DVG_ERR_SHAPE,
                "dvg_grad_sumsq: n = %ld must be a positive multiple of 4", n);
    DVG_REQUIRE(aligned16(g) && aligned_to<8>(partials), DVG_ERR_ALIGN,
                "dvg_grad_sumsq: g must be 16-byte aligned, partials 8-byte aligned");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)dvg_grad_sumsq_blocks(n)), dim3(GG_THREADS), 0, (hipStream_t)stream, g,
                       n >> 2, partials);
    return check_launch("dvg_grad_sumsq");
}

extern "C" int dvg_grad_guard_finish(const double* partials, int nblocks, double max_norm, int skip_nonfinite, float* stat,
                                     int* counters, void* stream) {
    DVG_REQUIRE(partials && stat && counters, DVG_ERR_NULL, "dvg_grad_guard_finish: NULL pointer");
    DVG_REQUIRE(nblocks > 0 && !(max_norm != max_norm), DVG_ERR_SHAPE, "dvg_grad_guard_finish: nblocks = %d, max_norm = %g",
                nblocks, max_norm);
    DVG_REQUIRE(aligned_to<8>(partials) && aligned_to<4>(stat) && aligned_to<4>(counters), DVG_ERR_ALIGN, "dvg_grad_guard_finish: misaligned buffer");
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(GG_THREADS), 0, (hipStream_t)stream, partials, nblocks, max_norm,
                       skip_nonfinite, stat, counters);
    return check_launch("dvg_grad_guard_finish");
}

// Gradient-norm clipping and the skip of a non-finite step, decided ON THE DEVICE (train.py --clip_grad_norm / --skip_nonfinite):
// the iteration is a captured hipGraph, so the host cannot look at a gradient between the backward pass and the Adam steps.
//
//   dvg_grad_sumsq         partials[b] = sum of squares of chunk b of a flat gradient range, fp64
//   dvg_grad_guard_finish  norm = sqrt(sum of the partials); stat = {norm, clip factor, skip, max finite norm}; counters
//   dvg_adam_step_guarded  dvg_adam_step on g * stat[1], or nothing at all when stat[2] != 0
//
// Arithmetic of the norm.  Every element is converted to fp64 and squared THERE: an fp32 x fp32 product is exact in fp64 (48
// of 53 significand bits, exponents within +-298), so no square overflows or underflows, and the sum of up to 2^25 finite
// squares (< 2^25 x 2^256) cannot overflow either.  "The fp64 sum is not finite" is therefore EXACTLY "some gradient is Inf or
// NaN": squares are >= 0, so Inf never meets -Inf, Inf stays Inf and NaN stays NaN under the additions.
//
// Order.  Workgroup b owns the fixed chunk [b * GG_CHUNK, (b + 1) * GG_CHUNK) - no grid-stride loop, no grid cap: the number of
// partials is a function of n alone (dvg_grad_sumsq_blocks).  A thread adds its 16-byte pieces in index order into four fp64
// sums (one per vector lane), those as (s0 + s1) + (s2 + s3), the 64 lanes of a wave by a halving tree of cross-lane moves,
// the four waves through LDS in wave order.  No atomics: the same input gives the same bits on every launch, rank and resume.
#include "dvg_common.h"

namespace dvg {

constexpr int GG_THREADS = 256;
constexpr int GG_PIECES = 16;                                  // 16-byte loads per thread
constexpr long GG_CHUNK = (long)GG_THREADS * GG_PIECES * 4;    // 16 384 floats per workgroup

// lane 0 of every wave ends with the wave's sum; always the same tree
__device__ __forceinline__ double gg_wave_sum(double s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    return s;
}

// thread 0 returns the workgroup's sum (four waves, in wave order); `red` holds 4 doubles
__device__ __forceinline__ double gg_block_sum(double s, double* red) {
    s = gg_wave_sum(s);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

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
    const double s = gg_block_sum((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One workgroup.  Thread t adds partials t, t + 256, ... in that order; then the same tree as above.
__global__ __launch_bounds__(GG_THREADS) void grad_guard_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                        double max_norm, int skip_nonfinite,
                                                                        float* __restrict__ stat, int* __restrict__ counters) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += GG_THREADS) s += partials[i];
    const double sum = gg_block_sum(s, red);
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

// a * b rounded on its own: never contracted into an add that follows (HIP's __fmul_rn is a plain product, which the default
// -ffp-contract=fast-honor-pragmas does fuse)
__device__ __forceinline__ float gg_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// adam_step_kernel (backward.hip) with the gradient scaled by stat[1] as it is read; nothing is touched when stat[2] != 0.
// The product g * scale is rounded on its own (gg_mul_rn), so scale = 1 leaves every later operation - the weight-decay
// multiply-add included - with the operands adam_step_kernel has: the same bits.
__global__ void adam_step_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                         float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                         const int* __restrict__ step_dev, int step_host, const float* __restrict__ stat,
                                         int* __restrict__ skips_dev) {
    if (stat[2] != 0.f) {            // uniform over the grid; this launch does not read *skips_dev
        if (blockIdx.x == 0 && threadIdx.x == 0) *skips_dev += 1;
        return;
    }
    const float scale = stat[1];
    // the counts (device or host) were advanced for the skipped steps too: the bias corrections use the steps really applied
    const int t = (step_dev ? *step_dev : step_host) - *skips_dev;
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    const float lr_over_bc1 = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gg = gg_mul_rn(gv[e], scale) + wd * pv[e];
            mv[e] = b1 * mv[e] + (1.f - b1) * gg;
            vv[e] = b2 * vv[e] + (1.f - b2) * gg * gg;
            pv[e] -= lr_over_bc1 * mv[e] / (sqrtf(vv[e]) * inv_sqrt_bc2 + eps);
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {   // tail
        const long i = (n4 << 2) + threadIdx.x;
        const float gg = gg_mul_rn(g[i], scale) + wd * p[i];
        const float mm = b1 * m[i] + (1.f - b1) * gg, vv = b2 * v[i] + (1.f - b2) * gg * gg;
        m[i] = mm;
        v[i] = vv;
        p[i] -= lr_over_bc1 * mm / (sqrtf(vv) * inv_sqrt_bc2 + eps);
    }
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
    DVG_REQUIRE(aligned16(g) && (reinterpret_cast<uintptr_t>(partials) & 7u) == 0, DVG_ERR_ALIGN,
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
    DVG_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stat) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(counters) & 3u) == 0,
                DVG_ERR_ALIGN, "dvg_grad_guard_finish: misaligned buffer");
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(GG_THREADS), 0, (hipStream_t)stream, partials, nblocks, max_norm,
                       skip_nonfinite, stat, counters);
    return check_launch("dvg_grad_guard_finish");
}

extern "C" int dvg_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                                     const float* stat, int* skips_dev, void* stream) {
    DVG_REQUIRE(param && grad && exp_avg && exp_avg_sq && stat && skips_dev, DVG_ERR_NULL, "dvg_adam_step_guarded: NULL pointer");
    DVG_REQUIRE(n > 0 && (step >= 1 || step_dev != nullptr), DVG_ERR_SHAPE, "dvg_adam_step_guarded: n=%ld step=%d", n, step);
    DVG_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq), DVG_ERR_ALIGN,
                "dvg_adam_step_guarded: buffers must be 16-byte aligned");
    DVG_REQUIRE(((reinterpret_cast<uintptr_t>(stat) | reinterpret_cast<uintptr_t>(skips_dev) |
                  reinterpret_cast<uintptr_t>(step_dev)) & 3u) == 0,
                DVG_ERR_ALIGN, "dvg_adam_step_guarded: stat, skips_dev and step_dev must be 4-byte aligned");
    long grid = ((n + 3) / 4 + 255) / 256;       // as dvg_adam_step's grid_for((n + 3) / 4)
    if (grid < 1) grid = 1;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(adam_step_guarded_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_dev, step, stat, skips_dev);
    return check_launch("dvg_adam_step_guarded");
}

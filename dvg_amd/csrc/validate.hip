// dvg_val_accumulate: the reduction of train.py --val_every.  make_gifs' metric arrays of one batch - ssim / psnr / mse, each
// (B, S, T) fp32: batch row, sample, predicted step - are folded into running per-step sums that stay on the device, so that a
// validation over K batches is K launches on one stream and ONE readback.  The reference has no counterpart: its train.py scores
// nothing, and generate_frames.py:188-189 picks the best sample on the host (np.argsort of the mean SSIM) for its figures only.
//
// Per batch row b: best[b] = the sample with the largest fp64 sum over t (from 0.0, t ascending) of ssim[b, s, t]; a NaN sum loses
// to every other, ties go to the lowest s, all NaN gives 0.  Two tracks per (metric, step):
//   track 0  v = metric[b, best[b], t], taken if finite;
//   track 1  u = the fp64 mean over the FINITE metric[b, s, t], s ascending; a row with none is left out.
// A taken value adds {v, v * v} to acc[track][metric][t] and 1 to cnt[track][metric][t].  The finite test is what keeps one +inf
// Finn PSNR (identical frames) or one NaN from turning a whole curve into inf / NaN.
//
// Form.  One 256-thread workgroup per step t.  A thread takes the rows b = tid, tid + 256, ... in ascending order and keeps 12 fp64
// sums and 6 counts of its own; the workgroup combines them with block_sum (the xor butterfly inside a wave, then the four wave
// sums left to right) and twelve + six threads each add one total to one output element.  The geometry is fixed - T workgroups of
// 256 - so the order of every sum is a function of (B, S, T) alone: no atomics, the same bits on every launch.  Every workgroup
// forms the best sample of its rows itself (S x T loads per row out of L2: the arrays are a few hundred KB at most) instead of
// waiting for another workgroup's; workgroup 0 writes them out.
#include "dvg_common.h"

namespace dvg {

constexpr int VAL_NT = 256;

__device__ __forceinline__ bool val_finite(double v) { return fabs(v) < __builtin_huge_val(); }   // false for NaN

__device__ __forceinline__ int val_best_sample(const float* __restrict__ row, int S, int T) {
    int best = 0;
    double best_sum = 0.0;
    bool have = false;
    for (int s = 0; s < S; ++s) {
        double sum = 0.0;
        for (int t = 0; t < T; ++t) sum += (double)row[(size_t)s * T + t];
        if (sum == sum && (!have || sum > best_sum)) {
            best = s;
            best_sum = sum;
            have = true;
        }
    }
    return best;
}

__global__ __launch_bounds__(VAL_NT) void val_accumulate_kernel(const float* __restrict__ ssim, const float* __restrict__ psnr,
                                                                const float* __restrict__ mse, int B, int S, int T,
                                                                double* __restrict__ acc, long long* __restrict__ cnt,
                                                                int* __restrict__ best) {
#pragma clang fp contract(off)
    __shared__ double red_d[12 * (VAL_NT / 64)];
    __shared__ long long red_n[6 * (VAL_NT / 64)];
    const int t = blockIdx.x;
    const float* metric[3] = {ssim, psnr, mse};
    double sums[12];          // [track][metric][sum, sum of squares]
    long long counts[6];      // [track][metric]
#pragma unroll
    for (int q = 0; q < 12; ++q) sums[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) counts[q] = 0;
    for (int b = threadIdx.x; b < B; b += VAL_NT) {
        const size_t row = (size_t)b * S * T;
        const int sb = val_best_sample(ssim + row, S, T);
        if (best != nullptr && blockIdx.x == 0) best[b] = sb;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float* p = metric[m] + row + t;
            const double v = (double)p[(size_t)sb * T];
            if (val_finite(v)) {
                sums[2 * m] += v;
                sums[2 * m + 1] += v * v;
                counts[m] += 1;
            }
            double tot = 0.0;
            int n = 0;
            for (int s = 0; s < S; ++s) {
                const double x = (double)p[(size_t)s * T];
                if (val_finite(x)) {
                    tot += x;
                    ++n;
                }
            }
            if (n > 0) {
                const double u = tot / (double)n;
                sums[6 + 2 * m] += u;
                sums[6 + 2 * m + 1] += u * u;
                counts[3 + m] += 1;
            }
        }
    }
    block_sum<VAL_NT>(sums, red_d);
    block_sum<VAL_NT>(counts, red_n);
    // acc [2][3][T][2], cnt [2][3][T]: one thread per output element of this step
    const int q = threadIdx.x;
    if (q < 12) {
        double* a = acc + ((size_t)(q >> 1) * T + t) * 2 + (q & 1);
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k == q) total = sums[k];      // (a register array is not indexed by a lane-dependent value)
        *a += total;
    } else if (q >= 64 && q < 70) {
        long long total = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k == q - 64) total = counts[k];
        cnt[(size_t)(q - 64) * T + t] += total;
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_val_accumulate(const float* ssim, const float* psnr, const float* mse, int B, int S, int T, double* acc,
                                  long long* cnt, int* best, void* stream) {
    DVG_REQUIRE(B >= 1 && S >= 1 && T >= 1, DVG_ERR_SHAPE, "dvg_val_accumulate: B, S and T must be >= 1 (got %d, %d, %d)", B, S, T);
    DVG_REQUIRE((long)B * S * T < (1L << 31), DVG_ERR_SHAPE, "dvg_val_accumulate: %d x %d x %d entries exceed 2^31 - 1", B, S, T);
    DVG_REQUIRE(ssim && psnr && mse && acc && cnt, DVG_ERR_NULL, "dvg_val_accumulate: NULL pointer (only `best` may be NULL)");
    hipLaunchKernelGGL(val_accumulate_kernel, dim3((unsigned)T), dim3(VAL_NT), 0, (hipStream_t)stream, ssim, psnr, mse, B, S, T,
                       acc, cnt, best);
    return check_launch("dvg_val_accumulate");
}

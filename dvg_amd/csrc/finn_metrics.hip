// dvg_eval_frames_finn: the metric set of utils.finn_eval_seq (utils.py:236-301), the variant the SVG / SV2P / DVG papers
// report KTH and BAIR with: per (frame, channel) image SSIM under an 11x11 Gaussian window (sigma 1.5, fspecial_gauss
// :270-273) over the (H-10)x(W-10) valid positions with K1 = 0.01, K2 = 0.03, L = 1 (finn_ssim :275-301), PSNR as
// 10 log10(1 / mse) (finn_psnr :259-261), and per frame the MSE over all channels (mse_metric :215-218).
//
// Form.  The window is the outer product of the normalised 1-D Gaussian, so the five moments (mu_x, mu_y, E[x^2], E[y^2],
// E[xy]) are filtered separably: a row pass (11 taps along x) into fp64 planes in LDS, then a column pass (11 taps along y)
// out of them - 11 + 11 taps per moment instead of 121.  Window sums, the E[x^2] - mu^2 differences and every reduction are
// fp64, as in eval_frames_kernel: the variance is a difference of nearly equal numbers set against C2 = 9e-4 and fp32
// cancels on flat regions (the Moving-MNIST background).
//
// LDS.  What is staged is the ROW-FILTERED STRIP, not the images.  Two 128x128 fp32 images are 128 KB of the 160 KB LDS and
// leave no room for five fp64 planes beside them, while the images themselves are read 11 times per row only, by
// neighbouring lanes at neighbouring addresses (the strip's input rows, <= 30 KB, stay in the vector L1).  So one workgroup
// takes one image in strips of rows_in <= 30 input rows = rows_in - 10 output rows: 5 x rows_in x (W-10) doubles, 65 KB at
// 64x64 (two workgroups per CU) and 142 KB at 128x128; the 10 halo rows of a strip are filtered again by the next one
// (x1.5 on the row pass at 20 output rows per strip).  Wider images get fewer rows per strip, down to the window's 11.
//
// Order.  Every lane sums its window positions in index order, the 64 lanes of a wave and then the four wave sums combine in a
// fixed tree (block_sum, pairwise: dvg_common.h): two launches give the same bits.  No atomics.
#include <cmath>

#include "dvg_common.h"

namespace dvg {

constexpr int FINN_WIN = 11;
constexpr int FINN_MAX_ROWS = 30;              // input rows per strip
constexpr size_t FINN_LDS_MAX = 150 * 1024;    // like eval_frames_kernel's tile

struct FinnTaps {
    double g[FINN_WIN];                        // exp(-i^2 / (2 sigma^2)) / sum, i = -5 ... 5
};

// utils.py:300-301 at one window position.  No contraction: with identical images 2 mu_x mu_y and mu_x^2 + mu_y^2 (and the
// two variance sums) must round alike, so that the ratio is exactly 1.
__device__ __forceinline__ double finn_ssim_point(double ux, double uy, double exx, double eyy, double exy) {
#pragma clang fp contract(off)
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double uxx = ux * ux, uyy = uy * uy, uxy = ux * uy;
    const double vx = exx - uxx, vy = eyy - uyy, vxy = exy - uxy;
    return ((2.0 * uxy + C1) * (2.0 * vxy + C2)) / ((uxx + uyy + C1) * (vx + vy + C2));
}

__device__ __forceinline__ double finn_sq_err(const float* __restrict__ a, const float* __restrict__ b, int n) {
    double se = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = (double)a[i] - (double)b[i];
        se += d * d;
    }
    return se;
}

// One workgroup per (frame, channel) image.  ssim / psnr: [n_frames * C]; mse: [n_frames], written by the workgroup of the
// frame's channel 0, which also sums the squared error of the frame's other channels (channel order, each reduced alike).
__global__ __launch_bounds__(256) void eval_frames_finn_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                               float* __restrict__ ssim, float* __restrict__ psnr,
                                                               float* __restrict__ mse, int C, int H, int W, int rows_in,
                                                               FinnTaps taps) {
    extern __shared__ __attribute__((aligned(16))) double rowf[];   // [5][rows_in][Wo]
    __shared__ double red[4];
    const int HW = H * W;
    const size_t base = (size_t)blockIdx.x * HW;
    const float* X = gt + base;
    const float* Y = pred + base;
    const int Ho = H - FINN_WIN + 1, Wo = W - FINN_WIN + 1;
    const int plane = rows_in * Wo;
    const int R = rows_in - FINN_WIN + 1;      // output rows per strip
    double ssum = 0.0;
    for (int y0 = 0; y0 < Ho; y0 += R) {       // uniform over the workgroup: the barriers are safe
        const int nin = min(rows_in, H - y0), nout = nin - FINN_WIN + 1;
        for (int e = threadIdx.x; e < nin * Wo; e += 256) {
            const int r = e / Wo, ox = e - r * Wo;
            const float* xr = X + (y0 + r) * W + ox;
            const float* yr = Y + (y0 + r) * W + ox;
            double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int k = 0; k < FINN_WIN; ++k) {
                const double a = xr[k], b = yr[k], g = taps.g[k];
                sx += g * a; sy += g * b; sxx += g * (a * a); syy += g * (b * b); sxy += g * (a * b);
            }
            rowf[e] = sx; rowf[plane + e] = sy; rowf[2 * plane + e] = sxx; rowf[3 * plane + e] = syy; rowf[4 * plane + e] = sxy;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < nout * Wo; o += 256) {
            double ux = 0, uy = 0, exx = 0, eyy = 0, exy = 0;
#pragma unroll
            for (int k = 0; k < FINN_WIN; ++k) {
                const double g = taps.g[k];
                const double* p = rowf + o + k * Wo;
                ux += g * p[0]; uy += g * p[plane]; exx += g * p[2 * plane]; eyy += g * p[3 * plane]; exy += g * p[4 * plane];
            }
            ssum += finn_ssim_point(ux, uy, exx, eyy, exy);
        }
        __syncthreads();                       // the next strip overwrites the planes
    }
    const double s = block_sum<256, SUM_PAIRWISE>(ssum, red);
    const double e = block_sum<256, SUM_PAIRWISE>(finn_sq_err(X, Y, HW), red);
    double frame_se = e;
    const int c = blockIdx.x % C;
    if (c == 0)
        for (int k = 1; k < C; ++k)
            frame_se += block_sum<256, SUM_PAIRWISE>(finn_sq_err(X + (size_t)k * HW, Y + (size_t)k * HW, HW), red);
    if (threadIdx.x == 0) {
        const double m = s / ((double)Ho * Wo);
        ssim[blockIdx.x] = m != m ? -1.f : (float)m;                       // utils.py:247-248: a NaN mean counts as -1
        psnr[blockIdx.x] = (float)(10.0 * log10(1.0 / (e / (double)HW)));   // data range 1 always; +inf for identical images
        if (c == 0) mse[blockIdx.x / C] = (float)(frame_se / ((double)C * HW));
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_eval_frames_finn(const float* gt, const float* pred, float* ssim, float* psnr, float* mse, int n_frames,
                                    int C, int H, int W, void* stream) {
    DVG_REQUIRE(gt && pred && ssim && psnr && mse, DVG_ERR_NULL, "dvg_eval_frames_finn: NULL pointer");
    DVG_REQUIRE(n_frames > 0 && C > 0, DVG_ERR_SHAPE, "dvg_eval_frames_finn: n_frames and C must be >= 1");
    DVG_REQUIRE(H >= FINN_WIN && W >= FINN_WIN, DVG_ERR_SHAPE,
                "dvg_eval_frames_finn: %dx%d images are smaller than the 11x11 Gaussian window", H, W);
    DVG_REQUIRE((long)n_frames * C * H * W < (1L << 31), DVG_ERR_SHAPE,
                "dvg_eval_frames_finn: %dx%dx%dx%d elements exceed the 32-bit offsets of the kernel", n_frames, C, H, W);
    const int Wo = W - FINN_WIN + 1;
    const size_t row_bytes = (size_t)5 * Wo * sizeof(double);
    const int rows_in = (int)std::min<size_t>(std::min(H, FINN_MAX_ROWS), FINN_LDS_MAX / row_bytes);
    DVG_REQUIRE(rows_in >= FINN_WIN, DVG_ERR_SHAPE,
                "dvg_eval_frames_finn: 11 row-filtered rows of a %d-wide image do not fit the LDS strip", W);
    const size_t lds = row_bytes * rows_in;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eval_frames_finn_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)FINN_LDS_MAX);
        if (e != hipSuccess) return fail(DVG_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    FinnTaps taps;
    double sum = 0.0;
    for (int i = 0; i < FINN_WIN; ++i) {
        const double d = i - FINN_WIN / 2;
        taps.g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += taps.g[i];
    }
    for (int i = 0; i < FINN_WIN; ++i) taps.g[i] /= sum;
    hipLaunchKernelGGL(eval_frames_finn_kernel, dim3((unsigned)(n_frames * C)), dim3(256), lds, (hipStream_t)stream, gt, pred,
                       ssim, psnr, mse, C, H, W, rows_in, taps);
    return check_launch("dvg_eval_frames_finn");
}

// dvg_frame_ssim_loss: the DSSIM frame term sum (1 - SSIM) of train.py --ssim_weight and its gradient in ONE launch, for the K decoder
// calls of every step against the step's target.  SSIM is the Finn SSIM of dvg_eval_frames_finn (finn_metrics.hip: 11x11 Gaussian
// window, sigma 1.5, K1 = 0.01, K2 = 0.03, L = 1, the (H-10) x (W-10) valid positions) - the number --val_every selects checkpoints
// by.  No reference counterpart: its train.py:227-239 is nn.MSELoss.  Definition, gradient and measurements:
// docs/DESIGN_NOTES_frame_loss.md.
//
//   pred [S][K][planes][H][W], target [S][planes][H][W]; x = T, y = P one plane, g the window, mu / e the filtered moments:
//     A1 = 2 mu_x mu_y + C1    A2 = 2 (e_xy - mu_x mu_y) + C2    B1 = mu_x^2 + mu_y^2 + C1    B2 = (e_xx - mu_x^2) + (e_yy - mu_y^2) + C2
//     S = A1 A2 / (B1 B2);   c = dS/de_xy = 2 A1 / (B1 B2);   b = dS/de_yy = -S / B2;
//     a = dS/dmu_y = 2 mu_x (A2 - A1) / (B1 B2) - 2 mu_y S / B1 + 2 mu_y S / B2
//     d(sum S)/dP[q] = full(a)[q] + 2 P[q] full(b)[q] + T[q] full(c)[q],   full = the transposed ("full"-mode) separable filter
//   sums[k] = sum (1 - S) of call k over steps, planes and positions;  dpred (+)= -w_ssim[k] d(sum S)/dP.
//
// fp64 between the fp32 loads and the fp32 stores: the variances are differences of nearly equal numbers set against C2 = 9e-4 (fp32
// misses the gradient by 2e-4 on constant images).  S has finn_ssim_point's contraction-off form: identical images give S = 1 exactly.
//
// Form.  One workgroup of 1024 threads per (step, plane, band of R pixel rows); R = H (the whole image) when that fits the LDS.  The band
// needs the maps at rows [y0 - 10, y0 + R) n [0, Ho): rows of a neighbour's band are computed again, not exchanged.  LDS, in fp64 rows
// of Wo = W - 10:  TM [2][MR] the target's mu_x, e_xx at the map rows, formed ONCE and reused by the K calls;  AB [3][MR] the call's
// a, b, c;  SR [3][RS] a strip: forward, the row-filtered moments of RS input rows (finn_metrics.hip's scheme: RS - 10 map rows per
// strip, the 10 halo rows filtered again by the next); backward, the column-transposed a, b, c of RS pixel rows, which the transposed row
// pass turns into 4-pixel vectors, fused with 2 P, T, the weight and the 16-byte store (a read-modify-write by the owner under
// `accumulate`).  A map position is SUMMED by the band that owns its pixel row.  Per workgroup one fp64 partial per call
// (block_sum over the 16 waves in wave order), finished in fp64 by one workgroup in a fixed tree: the same bits on every launch.  No atomics.
#include <algorithm>
#include <climits>
#include <cmath>

#include "dvg_common.h"

namespace dvg {

constexpr int SSL_WIN = 11, SSL_HALO = SSL_WIN - 1;
constexpr int SSL_STRIP_WHOLE = 30;            // strip rows when one workgroup takes the image (finn_metrics.hip's 30), fewer if LDS asks
constexpr int SSL_STRIP_BAND = 16;             // strip rows when the image is cut into bands; also the least a whole image must leave
constexpr size_t SSL_LDS_MAX = 150 * 1024;     // like eval_frames_finn_kernel's
constexpr int SSL_NT = 1024;                   // threads: the image's 150 KiB of LDS leave one workgroup per CU, so the waves that hide the
                                               // load, LDS and fp64 latencies must come from it: 0.83 / 0.54 / 0.46 ms at 256 / 512 / 1024 (design note)

struct SslTaps {
    double g[SSL_WIN];                         // exp(-i^2 / (2 sigma^2)) / sum, i = -5 ... 5
};

struct SslPlan {
    int R, RS, MR, bands;                      // pixel rows per band, strip rows, map rows held, bands per image; R = 0: not served
};

// A function of the shape alone.  `budget` = the fp64 rows of Wo that fit; held: 5 MR + 3 RS.
inline SslPlan ssl_plan(int H, int W) {
    SslPlan p = {0, 0, 0, 0};
    if (H < SSL_WIN || W < SSL_WIN || W % 4) return p;
    const int Ho = H - SSL_HALO, Wo = W - SSL_HALO;
    const long budget = (long)(SSL_LDS_MAX / (sizeof(double) * Wo));
    if (5L * Ho + 3L * std::min(H, SSL_STRIP_BAND) <= budget) {              // the whole image in one workgroup
        p.R = H;
        p.RS = (int)std::min<long>(std::min(H, SSL_STRIP_WHOLE), (budget - 5L * Ho) / 3);
    } else {
        p.RS = SSL_STRIP_BAND;
        long R = (budget - 3L * p.RS) / 5 - SSL_HALO;
        if (R < 1) {                                                         // a wide image: the window's 11 rows per strip
            p.RS = SSL_WIN;
            R = (budget - 3L * p.RS) / 5 - SSL_HALO;
        }
        if (R < 1) return SslPlan{0, 0, 0, 0};
        p.R = (int)std::min<long>(R, H);
    }
    p.MR = std::min(Ho, p.R + SSL_HALO);
    p.bands = (H + p.R - 1) / p.R;
    return p;
}

// S of finn_ssim_point (finn_metrics.hip), the same expression under the same pragma, and its partial derivatives a, b, c above.
__device__ __forceinline__ double ssl_point(double ux, double uy, double exx, double eyy, double exy, double& a, double& b, double& c) {
#pragma clang fp contract(off)
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double uxx = ux * ux, uyy = uy * uy, uxy = ux * uy;
    const double vx = exx - uxx, vy = eyy - uyy, vxy = exy - uxy;
    const double A1 = 2.0 * uxy + C1, A2 = 2.0 * vxy + C2, B1 = uxx + uyy + C1, B2 = vx + vy + C2;
    const double S = (A1 * A2) / (B1 * B2);
    const double inv = 1.0 / (B1 * B2);
    c = 2.0 * A1 * inv;
    b = -S / B2;
    a = 2.0 * ux * (A2 - A1) * inv - 2.0 * uy * S / B1 + 2.0 * uy * S / B2;
    return S;
}

__global__ __launch_bounds__(SSL_NT) void frame_ssim_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                              float* __restrict__ dpred, double* __restrict__ partial, int K,
                                                              long planes, int H, int W, SslPlan plan,
                                                              const float* __restrict__ w_ssim, int accumulate, SslTaps taps) {
    extern __shared__ __attribute__((aligned(16))) double ssl_lds[];   // TM [2][MR][Wo], AB [3][MR][Wo], SR [3][RS][Wo]
    __shared__ double red[SSL_NT / 64];
    const int Ho = H - SSL_HALO, Wo = W - SSL_HALO, W4 = W >> 2;
    const int R = plan.R, RS = plan.RS;
    const int mplane = plan.MR * Wo, splane = RS * Wo;
    double* TM = ssl_lds;
    double* AB = TM + 2 * mplane;
    double* SR = AB + 3 * mplane;
    const int band = (int)(blockIdx.x % (unsigned)plan.bands);
    const long sp = blockIdx.x / (unsigned)plan.bands, pl = sp % planes, s = sp / planes;
    const int y0 = band * R, y1 = min(y0 + R, H);                      // the pixel rows this workgroup owns
    const int m0 = max(0, y0 - SSL_HALO), m1 = min(Ho, y1);            // the map rows they depend on; m1 - m0 <= MR
    const long hw = (long)H * W;
    const float* T = target + (s * planes + pl) * hw;
    const int FS = RS - SSL_HALO;                                      // map rows per forward strip

    // the target's mu_x, e_xx at the map rows: once for the K calls (every loop bound is uniform over the workgroup)
    for (int ms = m0; ms < m1; ms += FS) {
        const int nout = min(FS, m1 - ms), nin = nout + SSL_HALO;
        for (int e = threadIdx.x; e < nin * Wo; e += SSL_NT) {
            const int r = e / Wo, ox = e - r * Wo;
            const float* xr = T + (ms + r) * W + ox;
            double sx = 0, sxx = 0;
#pragma unroll
            for (int k = 0; k < SSL_WIN; ++k) {
                const double v = xr[k], g = taps.g[k];
                sx = fma(g, v, sx); sxx = fma(g, v * v, sxx);   // explicit: the call's pass below must round alike
            }
            SR[e] = sx; SR[splane + e] = sxx;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < nout * Wo; o += SSL_NT) {
            double ux = 0, exx = 0;
#pragma unroll
            for (int k = 0; k < SSL_WIN; ++k) {
                const double g = taps.g[k];
                const double* p = SR + o + k * Wo;
                ux = fma(g, p[0], ux); exx = fma(g, p[splane], exx);
            }
            const int i = (ms - m0) * Wo + o;
            TM[i] = ux; TM[mplane + i] = exx;
        }
        __syncthreads();
    }

    for (int k = 0; k < K; ++k) {
        const long p0 = ((s * K + k) * planes + pl) * hw;
        const float* P = pred + p0;
        float* D = dpred + p0;
        // forward: the row-filtered moments of the call strip by strip, then S, a, b, c at the strip's map rows
        double ssum = 0.0;
        for (int ms = m0; ms < m1; ms += FS) {
            const int nout = min(FS, m1 - ms), nin = nout + SSL_HALO;
            for (int e = threadIdx.x; e < nin * Wo; e += SSL_NT) {
                const int r = e / Wo, ox = e - r * Wo;
                const float* xr = T + (ms + r) * W + ox;
                const float* yr = P + (ms + r) * W + ox;
                double sy = 0, syy = 0, sxy = 0;
#pragma unroll
                for (int t = 0; t < SSL_WIN; ++t) {
                    const double u = xr[t], v = yr[t], g = taps.g[t];
                    sy = fma(g, v, sy); syy = fma(g, v * v, syy); sxy = fma(g, u * v, sxy);
                }
                SR[e] = sy; SR[splane + e] = syy; SR[2 * splane + e] = sxy;
            }
            __syncthreads();
            for (int o = threadIdx.x; o < nout * Wo; o += SSL_NT) {
                double uy = 0, eyy = 0, exy = 0;
#pragma unroll
                for (int t = 0; t < SSL_WIN; ++t) {
                    const double g = taps.g[t];
                    const double* p = SR + o + t * Wo;
                    uy = fma(g, p[0], uy); eyy = fma(g, p[splane], eyy); exy = fma(g, p[2 * splane], exy);
                }
                const int i = (ms - m0) * Wo + o;
                double a, b, c;
                const double S = ssl_point(TM[i], uy, TM[mplane + i], eyy, exy, a, b, c);
                AB[i] = a; AB[mplane + i] = b; AB[2 * mplane + i] = c;
                if (ms + o / Wo >= y0) ssum += 1.0 - S;                 // rows above y0 are the upper neighbour's to sum
            }
            __syncthreads();
        }
        const double total = block_sum<SSL_NT, SUM_WAVE_ORDER>(ssum, red);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * K + k] = total;
        const double wk = (double)w_ssim[k];
        if (wk == 0.0 && accumulate) continue;                         // an exact 0 added: nothing to do (uniform)

        // backward: the transposed column pass into the strip, then the transposed row pass, 4 pixels per thread
        for (int rs = y0; rs < y1; rs += RS) {
            const int nb = min(RS, y1 - rs);
            for (int e = threadIdx.x; e < nb * Wo; e += SSL_NT) {
                const int rr = e / Wo, ox = e - rr * Wo, r = rs + rr;
                double fa = 0, fb = 0, fc = 0;
#pragma unroll
                for (int t = 0; t < SSL_WIN; ++t) {
                    const int m = r - t;                               // mu[m] took row r with tap t
                    if (m >= m0 && m < m1) {
                        const double g = taps.g[t];
                        const double* q = AB + (m - m0) * Wo + ox;
                        fa += g * q[0]; fb += g * q[mplane]; fc += g * q[2 * mplane];
                    }
                }
                SR[e] = fa; SR[splane + e] = fb; SR[2 * splane + e] = fc;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < nb * W4; i += SSL_NT) {
                const int rr = i / W4, x0 = 4 * (i - rr * W4);
                const double* col = SR + rr * Wo;
                double ga[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0}, gc[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = -SSL_HALO; j <= 3; ++j) {                  // map column x0 + j reaches pixel x0 + q with tap q - j
                    const int ox = x0 + j;
                    if (ox >= 0 && ox < Wo) {
                        const double va = col[ox], vb = col[splane + ox], vc = col[2 * splane + ox];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (q - j >= 0 && q - j < SSL_WIN) {
                                const double g = taps.g[q - j];
                                ga[q] += g * va; gb[q] += g * vb; gc[q] += g * vc;
                            }
                        }
                    }
                }
                const int o = (rs + rr) * W + x0;
                const f32x4 pv = *reinterpret_cast<const f32x4*>(P + o);
                const f32x4 tv = *reinterpret_cast<const f32x4*>(T + o);
                f32x4 out;
#pragma unroll
                for (int q = 0; q < 4; ++q) out[q] = (float)(-wk * (ga[q] + 2.0 * (double)pv[q] * gb[q] + (double)tv[q] * gc[q]));
                if (accumulate) out += *reinterpret_cast<const f32x4*>(D + o);
                *reinterpret_cast<f32x4*>(D + o) = out;
            }
            __syncthreads();                                           // the next strip overwrites SR
        }
    }
}

// sums[k] = the fp64 sum over the workgroups of partial[.][k]: frame_losses_ext_finish_kernel's tree on fp64 partials
__global__ __launch_bounds__(256) void frame_ssim_loss_finish_kernel(const double* __restrict__ partial, int blocks, int K,
                                                                     float* __restrict__ sums) {
    __shared__ double red[256];
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        for (int b = threadIdx.x; b < blocks; b += 256) a += partial[(size_t)b * K + k];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[k] = (float)red[0];
        __syncthreads();
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_frame_ssim_loss_blocks(int S, long planes, int H, int W) {
    if (S < 1 || planes < 1) return 0;
    const SslPlan p = ssl_plan(H, W);
    if (p.R == 0) return 0;
    const long g = (long)S * planes * p.bands;
    return g <= INT_MAX ? (int)g : 0;
}

extern "C" int dvg_frame_ssim_loss(const float* pred, const float* target, float* sums, float* dpred, int S, int K, long planes,
                                   int H, int W, const float* w_ssim, int accumulate, double* partial, void* stream) {
    DVG_REQUIRE(pred && target && sums && dpred && w_ssim && partial, DVG_ERR_NULL, "dvg_frame_ssim_loss: NULL pointer");
    DVG_REQUIRE(S > 0 && planes > 0 && H >= SSL_WIN && W >= SSL_WIN && W % 4 == 0 && K >= 1 && K <= 3, DVG_ERR_SHAPE,
                "dvg_frame_ssim_loss: H, W >= 11, W %% 4 == 0, K in 1..3 needed (S = %d, K = %d, planes = %ld, H = %d, W = %d)", S, K,
                planes, H, W);
    DVG_REQUIRE((double)S * K * (double)planes * H * W < 2147483648.0, DVG_ERR_SHAPE,
                "dvg_frame_ssim_loss: %dx%dx%ldx%dx%d elements exceed the 32-bit offsets of the kernel", S, K, planes, H, W);
    const SslPlan plan = ssl_plan(H, W);
    const int blocks = dvg_frame_ssim_loss_blocks(S, planes, H, W);
    DVG_REQUIRE(plan.R > 0 && blocks > 0, DVG_ERR_SHAPE,
                "dvg_frame_ssim_loss: the window's 11 rows of a %d-wide image do not fit the LDS strip", W);
    DVG_REQUIRE(aligned16(pred) && aligned16(target) && aligned16(dpred) && aligned_to<8>(partial), DVG_ERR_ALIGN,
                "dvg_frame_ssim_loss: alignment");
    const size_t lds = (size_t)(5 * plan.MR + 3 * plan.RS) * (W - SSL_HALO) * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&frame_ssim_loss_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)SSL_LDS_MAX);
        if (e != hipSuccess) return fail(DVG_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    SslTaps taps;
    double sum = 0.0;
    for (int i = 0; i < SSL_WIN; ++i) {
        const double d = i - SSL_WIN / 2;
        taps.g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += taps.g[i];
    }
    for (int i = 0; i < SSL_WIN; ++i) taps.g[i] /= sum;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_ssim_loss_kernel, dim3((unsigned)blocks), dim3(SSL_NT), lds, st, pred, target, dpred, partial, K, planes, H,
                       W, plan, w_ssim, accumulate, taps);
    if (int e = check_launch("dvg_frame_ssim_loss")) return e;
    hipLaunchKernelGGL(frame_ssim_loss_finish_kernel, dim3(1), dim3(256), 0, st, partial, blocks, K, sums);
    return check_launch("dvg_frame_ssim_loss (finish)");
}

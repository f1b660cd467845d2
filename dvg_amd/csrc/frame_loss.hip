// The frame terms of train_model's loss with a pixel term other than the square and / or the gradient-difference loss of Mathieu
// et al. (2016), and their gradient, in ONE pass (train.py --frame_loss / --gdl_weight).  No reference counterpart: its
// train.py:227-239 is plain nn.MSELoss, which dvg_frame_losses (misc_kernels.hip) stays the kernel for.  Definition and the
// decomposition below: docs/DESIGN_NOTES_frame_loss.md.
//
//   pred [S][K][planes][H][W] (per step the K decoder calls), target [S][planes][H][W]; P = one plane of one call, T = the
//   plane of the step's target, d = P - T:
//     pix_k = sum rho(d)          rho = d^2 | |d| | sqrt(d^2 + eps^2)                                  (kind 0 | 1 | 2)
//     gdl_k = sum_{x >= 1} | |P[y][x] - P[y][x-1]| - |T[y][x] - T[y][x-1]| |
//           + sum_{y >= 1} | |P[y][x] - P[y-1][x]| - |T[y][x] - T[y-1][x]| |                           (edges stay inside a plane)
//   sums [2][K] = pix, gdl over steps, planes and pixels;  dpred = d (sum_k w_pix[k] pix_k + w_gdl[k] gdl_k) / d pred, with
//   sign(0) = 0 everywhere (torch's abs): a tied edge - both differences equal in magnitude, the blank background of real frames -
//   contributes exactly 0.  A call whose w_gdl[k] is 0 gets no edge work: gdl_k = 0 exactly.
//
// One workgroup of 256 threads per (step, plane, band of R rows).  It stages the band of the target and of the K predictions in
// LDS - with one halo row above and below when any w_gdl is not 0 - by 16-byte loads, each byte of HBM once apart from the halo
// rows ((R + 2) / R on the reads).  Then every thread OWNS 4-pixel vectors of the band: it forms the target's four edge magnitudes
// once and reuses them for the K calls, and for each call reads the vector, its left / right neighbour pixels and the vectors above
// and below from LDS.  The gradient is in gather form: the owner adds the signed contributions of its pixel's up-to-4 edges, no
// atomics, no scatter.  An edge is SUMMED once, by the pixel with the larger coordinate: the horizontal edge (x-1, x) by x, the
// vertical edge (y-1, y) by y; halo rows contribute to gradients only.  Per-workgroup partial sums in a fixed order
// (block_sum, pairwise), reduced in fp64 by one finishing workgroup: the same bits on every launch.
#include <climits>
#include <cmath>

#include "dvg_common.h"

namespace dvg {

enum { FL_MSE = 0, FL_L1 = 1, FL_CHARBONNIER = 2 };   // `kind`, as include/dvg_hip.h numbers them
constexpr int FLX_MAX_ROWS = 16;                       // R for W <= 220
constexpr int FLX_BUF_FLOATS = 4000;                   // (R + 2) * W floats per staged tensor at most: 4 tensors + the sums < 64 KiB

// rows per band: 16, halved until the staged band fits (W = 256: 8, W = 512: 4, W = 1024: 1); 0 = no fit (W > 1332)
inline int flx_band_rows(int W) {
    int R = FLX_MAX_ROWS;
    while (R > 1 && (long)(R + 2) * W > FLX_BUF_FLOATS) R >>= 1;
    return (long)(R + 2) * W <= FLX_BUF_FLOATS ? R : 0;
}

__device__ __forceinline__ float fl_sign(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }

// |a| - m for the prediction's difference a across an edge whose target magnitude is m: adds |e| to `sum` when `count` (the
// edge is this pixel's to sum) and returns sign(e) sign(a), the derivative with respect to the pixel a was formed FROM (a = that
// pixel minus its neighbour); `valid` = false (no such edge in the plane): 0 and nothing summed.
__device__ __forceinline__ float fl_edge(float a, float m, bool valid, bool count, float& sum) {
    const float e = fabsf(a) - m;
    if (valid && count) sum += fabsf(e);
    return valid ? fl_sign(e) * fl_sign(a) : 0.f;
}

template <int K>
__global__ __launch_bounds__(256) void frame_losses_ext_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               float* __restrict__ dpred, float* __restrict__ partial, long planes,
                                                               int H, int W, int R, int bands, int kind, float eps2,
                                                               const float* __restrict__ w_pix, const float* __restrict__ w_gdl) {
    extern __shared__ __attribute__((aligned(16))) float fl_lds[];   // [1 + K][R + 2][W]: target, calls; then block_sum's 2 K x 4
    const int W4 = W >> 2, buf = (R + 2) * W;
    float* red = fl_lds + (1 + K) * buf;
    float wp[K], wg[K];
    bool any_gdl = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        wp[k] = w_pix[k];
        wg[k] = w_gdl[k];
        any_gdl |= wg[k] != 0.f;
    }
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const long sp = blockIdx.x / (unsigned)bands, plane = sp % planes, s = sp / planes;
    const int y0 = band * R, nr = min(R, H - y0);
    // LDS row r holds image row y0 - 1 + r; rows [rlo, rhi] exist and are staged
    const int rlo = (any_gdl && y0 > 0) ? 0 : 1, rhi = nr + ((any_gdl && y0 + nr < H) ? 1 : 0);
    const long hw = (long)H * W, band0 = (long)(y0 - 1) * W;
    const long t0 = (s * planes + plane) * hw + band0;
    long p0[K];
#pragma unroll
    for (int k = 0; k < K; ++k) p0[k] = ((s * K + k) * planes + plane) * hw + band0;

    const int nstage = (rhi - rlo + 1) * W4;
    for (int j = threadIdx.x; j < nstage; j += 256) {
        const int o = (rlo + j / W4) * W + 4 * (j % W4);
        const f32x4 t = *reinterpret_cast<const f32x4*>(target + t0 + o);
        f32x4 p[K];
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = *reinterpret_cast<const f32x4*>(pred + p0[k] + o);
        *reinterpret_cast<f32x4*>(fl_lds + o) = t;
#pragma unroll
        for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4*>(fl_lds + (1 + k) * buf + o) = p[k];
    }
    __syncthreads();

    float acc[2 * K];   // pix[K], gdl[K]
#pragma unroll
    for (int q = 0; q < 2 * K; ++q) acc[q] = 0.f;
    const int nown = nr * W4;
    for (int i = threadIdx.x; i < nown; i += 256) {
        const int r = 1 + i / W4, x0 = 4 * (i % W4), o = r * W + x0;
        const bool has_l = x0 > 0, has_r = x0 + 4 < W, has_u = y0 + r - 1 > 0, has_d = y0 + r < H;
        const f32x4 tc = *reinterpret_cast<const f32x4*>(fl_lds + o);
        float th[5], tu[4], td[4];   // the target's edge magnitudes: th[q] = edge (x0 + q - 1, x0 + q); up; down
        if (any_gdl) {
            const float tl = has_l ? fl_lds[o - 1] : 0.f, tr = has_r ? fl_lds[o + 4] : 0.f;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 ta = has_u ? *reinterpret_cast<const f32x4*>(fl_lds + o - W) : z;
            const f32x4 tb = has_d ? *reinterpret_cast<const f32x4*>(fl_lds + o + W) : z;
            th[0] = fabsf(tc[0] - tl);
            th[4] = fabsf(tr - tc[3]);
#pragma unroll
            for (int q = 1; q < 4; ++q) th[q] = fabsf(tc[q] - tc[q - 1]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                tu[q] = fabsf(tc[q] - ta[q]);
                td[q] = fabsf(tb[q] - tc[q]);
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float* lp = fl_lds + (1 + k) * buf;
            const f32x4 pc = *reinterpret_cast<const f32x4*>(lp + o);
            f32x4 g;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d = pc[q] - tc[q];
                if (kind == FL_MSE) {
                    acc[k] = fmaf(d, d, acc[k]);
                    g[q] = 2.f * wp[k] * d;
                } else if (kind == FL_L1) {
                    acc[k] += fabsf(d);
                    g[q] = wp[k] * fl_sign(d);
                } else {
                    const float rt = sqrtf(d * d + eps2);
                    acc[k] += rt;
                    g[q] = wp[k] * (d / rt);
                }
            }
            if (wg[k] != 0.f) {
                const float pl = has_l ? lp[o - 1] : 0.f, pr = has_r ? lp[o + 4] : 0.f;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 pa = has_u ? *reinterpret_cast<const f32x4*>(lp + o - W) : z;
                const f32x4 pb = has_d ? *reinterpret_cast<const f32x4*>(lp + o + W) : z;
                float sh[5];   // sign(e) sign(a) of the five horizontal edges that touch the vector; [4] is the next owner's to sum
                sh[0] = fl_edge(pc[0] - pl, th[0], has_l, true, acc[K + k]);
#pragma unroll
                for (int q = 1; q < 4; ++q) sh[q] = fl_edge(pc[q] - pc[q - 1], th[q], true, true, acc[K + k]);
                sh[4] = fl_edge(pr - pc[3], th[4], has_r, false, acc[K + k]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float su = fl_edge(pc[q] - pa[q], tu[q], has_u, true, acc[K + k]);
                    const float sd = fl_edge(pb[q] - pc[q], td[q], has_d, false, acc[K + k]);
                    // the pixel is the minuend of its left / upper edge and the subtrahend of its right / lower one
                    g[q] = fmaf(wg[k], (sh[q] - sh[q + 1]) + (su - sd), g[q]);
                }
            }
            *reinterpret_cast<f32x4*>(dpred + p0[k] + o) = g;
        }
    }
    block_sum<256, SUM_PAIRWISE>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 2 * K; ++q) partial[(size_t)blockIdx.x * (2 * K) + q] = acc[q];
    }
}

// sums[q] = the fp64 sum over the workgroups of partial[.][q], q < Q = 2 K: frame_losses_finish_kernel's tree (misc_kernels.hip)
__global__ __launch_bounds__(256) void frame_losses_ext_finish_kernel(const float* __restrict__ partial, int blocks, int Q,
                                                                      float* __restrict__ sums) {
    __shared__ double red[256];
    for (int q = 0; q < Q; ++q) {
        double a = 0.0;
        for (int b = threadIdx.x; b < blocks; b += 256) a += (double)partial[(size_t)b * Q + q];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[q] = (float)red[0];
        __syncthreads();
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_frame_losses_ext_blocks(int S, long planes, int H, int W) {
    if (S < 1 || planes < 1 || H < 1 || W < 4 || W % 4) return 0;
    const int R = flx_band_rows(W);
    if (R == 0) return 0;
    const long g = (long)S * planes * ((H + R - 1) / R);
    return g <= INT_MAX ? (int)g : 0;
}

extern "C" int dvg_frame_losses_ext(const float* pred, const float* target, float* sums, float* dpred, int S, int K, long planes,
                                    int H, int W, int kind, float eps, const float* w_pix, const float* w_gdl, float* partial,
                                    void* stream) {
    DVG_REQUIRE(pred && target && sums && dpred && w_pix && w_gdl && partial, DVG_ERR_NULL, "dvg_frame_losses_ext: NULL pointer");
    DVG_REQUIRE(S > 0 && planes > 0 && H >= 1 && W >= 4 && W % 4 == 0 && K >= 1 && K <= 3, DVG_ERR_SHAPE,
                "dvg_frame_losses_ext: W %% 4 == 0, W >= 4, H >= 1, K in 1..3 needed (S = %d, K = %d, planes = %ld, H = %d, W = %d)", S,
                K, planes, H, W);
    DVG_REQUIRE(kind >= FL_MSE && kind <= FL_CHARBONNIER, DVG_ERR_SHAPE, "dvg_frame_losses_ext: unknown kind %d", kind);
    DVG_REQUIRE(kind != FL_CHARBONNIER || (eps > 0.f && std::isfinite(eps)), DVG_ERR_SHAPE,
                "dvg_frame_losses_ext: charbonnier needs a finite eps = %g > 0", (double)eps);   // NaN fails
    const int R = flx_band_rows(W);
    const int blocks = dvg_frame_losses_ext_blocks(S, planes, H, W);
    DVG_REQUIRE(R > 0 && blocks > 0, DVG_ERR_SHAPE, "dvg_frame_losses_ext: W = %d above %d, or more than 2^31 - 1 bands", W,
                FLX_BUF_FLOATS / 3 / 4 * 4);
    DVG_REQUIRE(aligned16(pred) && aligned16(target) && aligned16(dpred), DVG_ERR_ALIGN, "dvg_frame_losses_ext: alignment");
    const int bands = (H + R - 1) / R;
    const size_t lds = ((size_t)(1 + K) * (R + 2) * W + 2 * K * 4) * sizeof(float);
    const float eps2 = eps * eps;
    hipStream_t st = (hipStream_t)stream;
#define DVG_FLX_LAUNCH(KK)                                                                                                      \
    hipLaunchKernelGGL(frame_losses_ext_kernel<KK>, dim3(blocks), dim3(256), lds, st, pred, target, dpred, partial, planes, H, W, R, \
                       bands, kind, eps2, w_pix, w_gdl)
    if (K == 1) DVG_FLX_LAUNCH(1);
    else if (K == 2) DVG_FLX_LAUNCH(2);
    else DVG_FLX_LAUNCH(3);
#undef DVG_FLX_LAUNCH
    if (int e = check_launch("dvg_frame_losses_ext")) return e;
    hipLaunchKernelGGL(frame_losses_ext_finish_kernel, dim3(1), dim3(256), 0, st, partial, blocks, 2 * K, sums);
    return check_launch("dvg_frame_losses_ext (finish)");
}

// dvg_pairwise_frame_mse: how different the nsample rollouts of make_gifs are from EACH OTHER.  The reference draws them in
// the sample loop generate_frames.py:147-183 and scores every one against the ground truth only (:178); it computes nothing
// between samples.  Per frame (step, batch row) this is the S x S matrix out[i][j] = mean_d (x_i[d] - x_j[d])^2.
//
// Form.  An SGEMM with (a - b)^2 in place of a * b, and it has to stay that: most pairs are identical or nearly so (every step
// before the first GP trigger step is the same computation for all samples), where the Gram form |a|^2 + |b|^2 - 2 a.b cancels
// to noise.  Every term here is the fp32 difference, squared; bit-identical frames give exactly 0.
//
// Tiling.  One 256-thread workgroup per (frame, upper-triangular tile block): TILE x TILE pairs, a thread keeps R x R of them
// (rows ty + 16 r against rows tx + 16 c) - R = 4, TILE = 64, or R = 2, TILE = 32 when S <= 32 (a 64-row tile would be mostly
// padding).  The two row tiles are staged in LDS in slabs of DC = 32 elements, [row][DC + 4]: a row stride of 9 16-byte slots,
// odd, so the 16 lanes of a ds_read_b128 group (16 consecutive rows, same column) hit 16 distinct slots, and the rows a wave
// shares are broadcasts.  Per 4 elements a thread issues 2 R b128 reads for 4 R^2 pair-elements.  The next slab's global loads
// are in flight while the current one is consumed.
//
// Arithmetic.  Per pair two fp32 partial sums (the even and the odd elements: one packed subtract and one packed FMA per two
// elements) over CHUNK = 256 consecutive elements, in element order; both are then added to the pair's fp64 sum, and the
// division by D is fp64.  Worst-case relative error against exact arithmetic on the same inputs: (128 + 4) 2^-24, inside the
// (256 + 4) 2^-24 of a single 256-term fp32 chunk.  Fixed order, no atomics: two launches give the same bits.  Only i < j is
// computed, and written to [i][j] and [j][i]; the diagonal is written as 0.  Rows past S repeat row S - 1 and elements past D
// are zero on both sides (their results are not written / add exactly 0).
#include "dvg_common.h"

namespace dvg {

constexpr int DIV_DC = 32;                 // elements per LDS slab
constexpr int DIV_LD = DIV_DC + 4;         // floats per LDS row
constexpr int DIV_CHUNK = 256;             // elements per fp32 partial sum (two interleaved halves)

// a - b on both halves as ONE v_pk_add_f32 with b negated (the same IEEE subtraction as v_sub_f32, two per instruction); the
// compiler turns a two-element vector subtraction into two v_sub_f32
__device__ __forceinline__ f32x2_t div_pk_sub(f32x2_t a, f32x2_t b) {
    f32x2_t d;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// VEC: D, both strides and the base are multiples of 4 floats / 16 bytes - 16-byte global loads; else element loads
template <int R, bool VEC>
__device__ __forceinline__ void div_load(f32x4* __restrict__ regs, const float* __restrict__ frame, long sample_stride, int S,
                                         int D, int row0a, int row0b, int d0) {
    constexpr int NL = R / 2;              // 16-byte pieces per thread and tile: TILE * 8 / 256
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int idx = (int)threadIdx.x + 256 * k;
            const int row = min((t ? row0b : row0a) + (idx >> 3), S - 1);
            const int d = d0 + (idx & 7) * 4;
            const float* p = frame + (size_t)row * sample_stride + d;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                if (d < D) v = *reinterpret_cast<const f32x4*>(p);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (d + e < D) v[e] = p[e];
            }
            regs[t * NL + k] = v;
        }
    }
}

template <int R, bool VEC>
__global__ __launch_bounds__(256) void pairwise_frame_mse_kernel(const float* __restrict__ samples, float* __restrict__ out,
                                                                 int S, long sample_stride, long frame_stride, int D,
                                                                 int n_tiles, int n_blocks) {
    constexpr int TILE = 16 * R, NL = R / 2;
    __shared__ __attribute__((aligned(16))) float As[TILE * DIV_LD];
    __shared__ __attribute__((aligned(16))) float Bs[TILE * DIV_LD];
    // workgroups of one frame are neighbours in the logical order and share an XCD's L2 (xcd_remap)
    const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
    const int f = (int)(lid / (unsigned)n_blocks);
    int blk = (int)(lid % (unsigned)n_blocks), bi = 0;
    while (blk >= n_tiles - bi) {          // upper-triangular block (bi, bj), bi <= bj
        blk -= n_tiles - bi;
        ++bi;
    }
    const int bj = bi + blk;
    const int row0a = bi * TILE, row0b = bj * TILE;
    const float* frame = samples + (size_t)f * frame_stride;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;

    f32x2_t acc[R][R];
    double sum[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) {
            acc[r][c] = f32x2_t{0.f, 0.f};
            sum[r][c] = 0.0;
        }

    f32x4 regs[2 * NL];
    div_load<R, VEC>(regs, frame, sample_stride, S, D, row0a, row0b, 0);
    int in_chunk = 0;
    for (int d0 = 0; d0 < D; d0 += DIV_DC) {
        __syncthreads();                   // the previous slab has been consumed
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int idx = (int)threadIdx.x + 256 * k;
            const int o = (idx >> 3) * DIV_LD + (idx & 7) * 4;
            *reinterpret_cast<f32x4*>(As + o) = regs[k];
            *reinterpret_cast<f32x4*>(Bs + o) = regs[NL + k];
        }
        __syncthreads();
        if (d0 + DIV_DC < D) div_load<R, VEC>(regs, frame, sample_stride, S, D, row0a, row0b, d0 + DIV_DC);
#pragma unroll
        for (int k4 = 0; k4 < DIV_DC / 4; ++k4) {
            f32x4 a[R], b[R];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = *reinterpret_cast<const f32x4*>(As + (ty + 16 * r) * DIV_LD + k4 * 4);
#pragma unroll
            for (int c = 0; c < R; ++c) b[c] = *reinterpret_cast<const f32x4*>(Bs + (tx + 16 * c) * DIV_LD + k4 * 4);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < R; ++c) {
                    const f32x2_t lo = div_pk_sub(f32x2_t{a[r][0], a[r][1]}, f32x2_t{b[c][0], b[c][1]});
                    acc[r][c] = __builtin_elementwise_fma(lo, lo, acc[r][c]);
                    const f32x2_t hi = div_pk_sub(f32x2_t{a[r][2], a[r][3]}, f32x2_t{b[c][2], b[c][3]});
                    acc[r][c] = __builtin_elementwise_fma(hi, hi, acc[r][c]);
                }
        }
        in_chunk += DIV_DC;
        if (in_chunk == DIV_CHUNK || d0 + DIV_DC >= D) {     // uniform over the grid
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < R; ++c) {
                    sum[r][c] += (double)acc[r][c][0] + (double)acc[r][c][1];
                    acc[r][c] = f32x2_t{0.f, 0.f};
                }
            in_chunk = 0;
        }
    }

    float* o = out + (size_t)f * S * S;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int i = row0a + ty + 16 * r, j = row0b + tx + 16 * c;
            if (i >= S || j >= S) continue;
            if (i < j) {
                const float v = (float)(sum[r][c] / (double)D);
                o[(size_t)i * S + j] = v;
                o[(size_t)j * S + i] = v;
            } else if (i == j) {
                o[(size_t)i * S + i] = 0.f;
            }
        }
}

template <int R, bool VEC>
static void div_launch(const float* samples, float* out, int S, long sample_stride, int frames, long frame_stride, int D,
                       int n_tiles, hipStream_t stream) {
    const int n_blocks = n_tiles * (n_tiles + 1) / 2;
    hipLaunchKernelGGL((pairwise_frame_mse_kernel<R, VEC>), dim3((unsigned)frames * (unsigned)n_blocks), dim3(256), 0, stream,
                       samples, out, S, sample_stride, frame_stride, D, n_tiles, n_blocks);
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_pairwise_frame_mse(const float* samples, float* out, int S, long sample_stride, int frames, long frame_stride,
                                      int D, void* stream) {
    DVG_REQUIRE(samples && out, DVG_ERR_NULL, "dvg_pairwise_frame_mse: NULL pointer");
    DVG_REQUIRE(S >= 1 && frames >= 1 && D >= 1, DVG_ERR_SHAPE, "dvg_pairwise_frame_mse: S, frames and D must be >= 1");
    DVG_REQUIRE(frame_stride >= D && (S == 1 || sample_stride >= D), DVG_ERR_SHAPE,
                "dvg_pairwise_frame_mse: strides %ld / %ld are below the frame's %d floats", sample_stride, frame_stride, D);
    const int tile = S <= 32 ? 32 : 64;
    const long n_tiles = (S + tile - 1) / tile, n_blocks = n_tiles * (n_tiles + 1) / 2;
    DVG_REQUIRE(n_blocks * frames < (1L << 31), DVG_ERR_SHAPE,
                "dvg_pairwise_frame_mse: %d frames x %ld tile blocks exceed the grid", frames, n_blocks);
    const bool vec = D % 4 == 0 && sample_stride % 4 == 0 && frame_stride % 4 == 0 && aligned16(samples);
    hipStream_t st = (hipStream_t)stream;
    if (tile == 32) {
        if (vec) div_launch<2, true>(samples, out, S, sample_stride, frames, frame_stride, D, (int)n_tiles, st);
        else div_launch<2, false>(samples, out, S, sample_stride, frames, frame_stride, D, (int)n_tiles, st);
    } else {
        if (vec) div_launch<4, true>(samples, out, S, sample_stride, frames, frame_stride, D, (int)n_tiles, st);
        else div_launch<4, false>(samples, out, S, sample_stride, frames, frame_stride, D, (int)n_tiles, st);
    }
    return check_launch("dvg_pairwise_frame_mse");
}

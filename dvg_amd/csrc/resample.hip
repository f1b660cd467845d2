// Frames of any size into the frame pool (`--resize`, dvg_amd/datasets.py build_pool): Pillow's 8-bit resampler, bit for bit.
//
// dvg_resample_u8: src (n,Hin,Win,C) uint8 -> dst (n,Hout,Wout,C) uint8, C = 1 or 3 interleaved.  As ImagingResample does it: a
// horizontal pass into a uint8 intermediate, then a vertical pass, each  clamp((2^21 + sum_k pixel * coef) >> 22, 0, 255)  in
// int32 over the integer coefficients the host derives as Pillow does (dvg_amd/resample.py); a pass with ksize 0 is a copy
// (Pillow skips a pass when the size stays and the box is the whole axis).  The crop box lives in the tables: xmin / ymin are
// absolute input positions.  dvg_mnist_scale_u8 (mnist.hip) is the square, up-scaling, bilinear case and stays as it is.
//
// One workgroup = one (frame, band of output rows [o0, o1)).  The horizontal pass covers only the input rows the band needs,
// ymin[o0] .. ymin[o1-1] + yk clipped to the image (Pillow computes ybox_first .. ybox_last only), and leaves its uint8 result
// in LDS; the vertical pass reads it there and writes the band's rows of dst, which are one contiguous run, four bytes per
// store.  Each wave takes one source row at a time: the columns the tables name are staged into the wave's LDS row with 4-byte
// loads (a source byte is read from memory about once), the taps then come from LDS.
//
// LDS budget: RESAMPLE_LDS = 64 KB per workgroup - the most a launch gets without an attribute call, and two workgroups still
// share a CU's 160 KB.  It holds the four row buffers (4 x (Win * C + 8) bytes, rounded to 16) and the intermediate (span rows of
// Wout * C bytes, span = the most input rows a band needs).  dvg_resample_u8_band chooses the largest band height whose
// intermediate fits, from the HOST copy of ymin; a geometry whose one-row band does not fit is refused before any launch.
//
// Table contents are device data: the first tap is clamped into the line, taps past its end - or outside what was staged -
// are skipped, and the band's row range is cut to the LDS rows it was given, so a bad table cannot read or write out of bounds.
#include "dvg_common.h"

namespace dvg {

constexpr int RESAMPLE_LDS = 64 * 1024;
constexpr int RESAMPLE_NT = 256;
constexpr int RESAMPLE_WAVES = RESAMPLE_NT / 64;
constexpr int RESAMPLE_PREC = 22;            // Pillow's PRECISION_BITS = 32 - 8 - 2

__host__ __device__ inline int resample_rowbuf_bytes(int Win, int C) { return (Win * C + 8 + 15) & ~15; }

__device__ __forceinline__ unsigned char resample_clip8(int acc) {
    const int v = acc >> RESAMPLE_PREC;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One output byte of the vertical pass: output row o, byte `col` of the row (mid rows are WC bytes, row r0 is mid's first).
__device__ __forceinline__ unsigned char resample_vertical(const unsigned char* mid, int WC, int col, int o, int Hin, int r0,
                                                           int rows, const int* __restrict__ ymin,
                                                           const int* __restrict__ ycoef, int yk) {
    if (yk == 0) return (unsigned)(o - r0) < (unsigned)rows ? mid[(o - r0) * WC + col] : (unsigned char)0;   // a copy
    const int y0 = clampi(ymin[o], 0, Hin - 1);
    int acc = 1 << (RESAMPLE_PREC - 1);
    for (int k = 0; k < yk; ++k) {
        const int rr = y0 + k - r0;
        if ((unsigned)rr < (unsigned)rows) acc += (int)mid[rr * WC + col] * ycoef[(size_t)o * yk + k];
    }
    return resample_clip8(acc);
}

__global__ __launch_bounds__(RESAMPLE_NT) void resample_u8_kernel(
    const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int Hin, int Win, int Hout, int Wout, int C,
    const int* __restrict__ xmin, const int* __restrict__ xcoef, int xk, const int* __restrict__ ymin,
    const int* __restrict__ ycoef, int yk, int band, int nbands, int span, size_t src_bytes, int src_dwords_ok) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int rowbuf = resample_rowbuf_bytes(Win, C);
    unsigned char* mid = lds + RESAMPLE_WAVES * rowbuf;            // [span][Wout * C]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* row = lds + wave * rowbuf;
    const size_t frame = blockIdx.x / (unsigned)nbands;
    const int o0 = (int)(blockIdx.x % (unsigned)nbands) * band;
    const int o1 = min(o0 + band, Hout);
    const int WC = Wout * C;

    // the input rows [r0, r0 + rows) this band needs, cut to the `span` rows of LDS the launch has
    int r0, rows;
    if (yk == 0) {
        r0 = o0;
        rows = min(o1, Hin) - o0;
    } else {
        r0 = clampi(ymin[o0], 0, Hin - 1);
        rows = min(clampi(ymin[o1 - 1], 0, Hin - 1) + yk, Hin) - r0;
    }
    rows = clampi(rows, 0, span);

    // the input columns [c0, c1) the horizontal pass reads
    int c0 = 0, c1 = Win;
    if (xk > 0) {
        c0 = clampi(xmin[0], 0, Win - 1);
        c1 = clampi(min(clampi(xmin[Wout - 1], 0, Win - 1) + xk, Win), c0 + 1, Win);
    }

    // ---- horizontal pass: wave w takes the rows r0 + w, r0 + w + 4, ... ------------------------------------------------------
    for (int base = 0; base < rows; base += RESAMPLE_WAVES) {      // uniform over the workgroup: the barriers are met by all
        const int rr = base + wave;
        size_t a0 = 0;
        if (rr < rows) {
            const size_t b0 = ((frame * Hin + (size_t)(r0 + rr)) * Win + c0) * C, b1 = b0 + (size_t)(c1 - c0) * C;
            a0 = src_dwords_ok ? (b0 & ~(size_t)3) : b0;           // row[i - a0] = src[i] for b0 <= i < b1
            if (src_dwords_ok) {
                for (size_t i = a0 + (size_t)lane * 4; i < b1; i += 64 * 4) {
                    if (i + 4 <= src_bytes) {
                        *reinterpret_cast<unsigned*>(row + (i - a0)) = *reinterpret_cast<const unsigned*>(src + i);
                    } else {
                        for (int j = 0; j < 4; ++j)
                            if (i + j < src_bytes) row[i - a0 + j] = src[i + j];
                    }
                }
            } else {
                for (size_t i = b0 + lane; i < b1; i += 64) row[i - b0] = src[i];
            }
        }
        __syncthreads();
        if (rr < rows) {
            const size_t b0 = ((frame * Hin + (size_t)(r0 + rr)) * Win + c0) * C;
            const unsigned char* line = row + (b0 - a0);           // line[(x - c0) * C + c] = the row's pixel x, channel c
            unsigned char* m = mid + (size_t)rr * WC;
            for (int j = lane; j < WC; j += 64) {
                const int x = j / C, c = j - x * C;
                if (xk == 0) {                                     // Wout == Win and the whole axis: a copy
                    m[j] = line[j];
                    continue;
                }
                const int x0 = clampi(xmin[x], 0, Win - 1);
                int acc = 1 << (RESAMPLE_PREC - 1);
                for (int k = 0; k < xk; ++k) {
                    const int xx = x0 + k;
                    if (xx >= c0 && xx < c1) acc += (int)line[(xx - c0) * C + c] * xcoef[(size_t)x * xk + k];
                }
                m[j] = resample_clip8(acc);
            }
        }
        __syncthreads();
    }

    // ---- vertical pass: the band's rows of dst are one contiguous run of bytes -----------------------------------------------
    const size_t d0 = (frame * Hout + (size_t)o0) * WC;
    const int len = (o1 - o0) * WC;
    const bool dwords = ((reinterpret_cast<uintptr_t>(dst) + d0) & 3) == 0;
    for (int q = tid * 4; q < len; q += RESAMPLE_NT * 4) {
        unsigned char v[4];
        const int nq = min(4, len - q);
        for (int j = 0; j < nq; ++j) {
            const int o = o0 + (q + j) / WC, col = (q + j) % WC;
            v[j] = resample_vertical(mid, WC, col, o, Hin, r0, rows, ymin, ycoef, yk);
        }
        if (dwords && nq == 4) {
            *reinterpret_cast<unsigned*>(dst + d0 + q) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
        } else {
            for (int j = 0; j < nq; ++j) dst[d0 + q + j] = v[j];
        }
    }
}

// The most input rows a band of `band` output rows needs (the HOST copy of ymin; yk == 0: the band itself).
static int resample_span(const int* ymin_host, int Hin, int Hout, int yk, int band) {
    if (yk == 0) return band < Hout ? band : Hout;
    int span = 1;
    for (int o0 = 0; o0 < Hout; o0 += band) {
        const int o1 = o0 + band < Hout ? o0 + band : Hout;
        int a = ymin_host[o0], b = ymin_host[o1 - 1];
        a = a < 0 ? 0 : (a > Hin - 1 ? Hin - 1 : a);
        b = b < 0 ? 0 : (b > Hin - 1 ? Hin - 1 : b);
        const int r1 = b + yk < Hin ? b + yk : Hin;
        if (r1 - a > span) span = r1 - a;
    }
    return span;
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_resample_u8_band(const int* ymin_host, int Hin, int Win, int Hout, int Wout, int C, int yk, int* span) {
    DVG_REQUIRE(Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1 && (C == 1 || C == 3) && yk >= 0, DVG_ERR_SHAPE,
                "dvg_resample_u8_band: sizes must be >= 1, C 1 or 3");
    DVG_REQUIRE(yk == 0 || ymin_host, DVG_ERR_NULL, "dvg_resample_u8_band: NULL ymin with a vertical pass");
    if (span) *span = 0;
    const long fixed = (long)RESAMPLE_WAVES * (((long)Win * C + 8 + 15) & ~15L);
    const long row = (long)Wout * C;
    for (int nb = 1; nb <= Hout; ++nb) {                           // the fewest, equal bands whose intermediate fits
        const int band = (Hout + nb - 1) / nb;
        if (nb > 1 && band == (Hout + nb - 2) / (nb - 1)) continue;
        const int s = resample_span(ymin_host, Hin, Hout, yk, band);
        if (fixed + (long)s * row <= RESAMPLE_LDS) {
            if (span) *span = s;
            return band;
        }
    }
    return 0;
}

extern "C" int dvg_resample_u8(const uint8_t* src, uint8_t* dst, int n, int Hin, int Win, int Hout, int Wout, int C,
                               const int* xmin, const int* xcoef, int xk, const int* ymin, const int* ycoef, int yk,
                               const int* ymin_host, void* stream) {
    DVG_REQUIRE(src && dst, DVG_ERR_NULL, "dvg_resample_u8: NULL pointer");
    DVG_REQUIRE(n >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1, DVG_ERR_SHAPE, "dvg_resample_u8: n and the sizes must be >= 1");
    DVG_REQUIRE(C == 1 || C == 3, DVG_ERR_SHAPE, "dvg_resample_u8: C = %d: 1 or 3 interleaved channels", C);
    DVG_REQUIRE(xk >= 0 && yk >= 0, DVG_ERR_SHAPE, "dvg_resample_u8: negative table size");
    DVG_REQUIRE(xk == 0 || (xmin && xcoef), DVG_ERR_NULL, "dvg_resample_u8: NULL table of the horizontal pass");
    DVG_REQUIRE(yk == 0 || (ymin && ycoef && ymin_host), DVG_ERR_NULL, "dvg_resample_u8: NULL table of the vertical pass");
    DVG_REQUIRE(xk > 0 || Wout == Win, DVG_ERR_SHAPE, "dvg_resample_u8: no horizontal pass, but %d -> %d columns", Win, Wout);
    DVG_REQUIRE(yk > 0 || Hout == Hin, DVG_ERR_SHAPE, "dvg_resample_u8: no vertical pass, but %d -> %d rows", Hin, Hout);
    DVG_REQUIRE((long)Win * C < (1L << 30) && (long)Wout * C < (1L << 30) && (long)Wout * xk < (1L << 30) &&
                (long)Hout * yk < (1L << 30), DVG_ERR_SHAPE, "dvg_resample_u8: a row or a table beyond 2^30 entries");
    // src offsets are 64-bit (4096 frames of 1080p exceed 2^31 bytes); the whole of either tensor stays below 2^46 bytes
    DVG_REQUIRE((double)n * Hin * Win * C < (double)(1L << 46) && (double)n * Hout * Wout * C < (double)(1L << 46), DVG_ERR_SHAPE,
                "dvg_resample_u8: tensor too large");
    int span = 0;
    const int band = dvg_resample_u8_band(ymin_host, Hin, Win, Hout, Wout, C, yk, &span);
    DVG_REQUIRE(band >= 1, DVG_ERR_SHAPE,
                "dvg_resample_u8: %dx%dx%d -> %dx%d: the input rows of ONE output row (%d taps of %d bytes) and four source rows do "
                "not fit %d KB of LDS", Hin, Win, C, Hout, Wout, yk ? yk : 1, Wout * C, RESAMPLE_LDS / 1024);
    const int nbands = (Hout + band - 1) / band;
    DVG_REQUIRE((long)n * nbands < (1L << 31), DVG_ERR_SHAPE, "dvg_resample_u8: %d frames x %d bands: too many workgroups", n, nbands);
    const size_t lds = (size_t)RESAMPLE_WAVES * resample_rowbuf_bytes(Win, C) + (size_t)span * Wout * C;
    const size_t src_bytes = (size_t)n * Hin * Win * C;
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)((long)n * nbands)), dim3(RESAMPLE_NT), lds, (hipStream_t)stream, src, dst,
                       Hin, Win, Hout, Wout, C, xmin, xcoef, xk, ymin, ycoef, yk, band, nbands, span, src_bytes,
                       (int)aligned_to<4>(src));
    return check_launch("dvg_resample_u8");
}

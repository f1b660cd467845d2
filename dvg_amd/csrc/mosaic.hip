// dvg_frame_mosaic: the figures of the reference (generate_frames.py:185-217 make_gifs, :235-245 plot_rec, train.py:291-335
// plot) composed on the device as uint8 RGB mosaics.  One launch does what utils.image_tensor (utils.py:104-150: grid on a
// canvas of ones), add_border (generate_frames.py:306-319: coloured cell, image inside, one channel replicated to three),
// draw_text_tensor (utils.py:167-173: black label pixels, bytes = uint8(v * 255)) and make_image (utils.py:160-165) do with
// .cpu() tensors and Python loops, and it resolves "the best sample of batch row b" from the index tensor where it lives.
// HBM-bound: every selected source pixel is read once, every mosaic byte written once.
#include "dvg_common.h"

namespace dvg {

struct MosaicArgs {
    const float* src[3];
    long n_img[3];
    const int* cells;
    const long* best;
    const int* picks;
    const unsigned char* labels;
    unsigned char* out;
    int nc, H, W;
    int F, R, Cc, cell_h, cell_w, pad_y, pad_x, oy, ox;
    int n_best, n_pick_rows, pick_k;
    int n_labels, lh, lw;
    int quant;
    unsigned GH, GW;
};

// clamp, scale, (round): the product and the add are two fp32 roundings (__fmul_rn / __fadd_rn are never contracted into
// an fma: fma(v, 255, 0.5) differs from the reference's numpy arithmetic on ties such as 0.7f * 255 = 178.5)
__device__ __forceinline__ unsigned quant_byte(float v, int quant) {
    v = fminf(fmaxf(v, 0.f), 1.f);
    float s = __fmul_rn(v, 255.f);
    if (quant == DVG_QUANT_NEAREST) s = __fadd_rn(s, 0.5f);
    return (unsigned)s;   // 0 <= s <= 255.5: truncation
}

// One resolved cell: where its image lives (NULL = background only), its background bytes, its label mask (NULL = none).
struct MosaicCell {
    const float* img;
    const unsigned char* label;
    unsigned bg;   // packed R | G << 8 | B << 16
};

__device__ __forceinline__ MosaicCell resolve_cell(const MosaicArgs& a, unsigned f, unsigned gy, unsigned gx) {
    const int* c = a.cells + ((size_t)(f * a.R + gy) * a.Cc + gx) * DVG_MOSAIC_CELL_INTS;
    const int src = c[0], base = c[1], stride = c[2], sel = c[3], b = c[4], k = c[5], colour = c[6], label = c[7];
    MosaicCell r;
    const float bgv = 0.7f;                                    // add_border: px[0] = 0.7 / px[1] = 0.7
    const unsigned q = quant_byte(bgv, a.quant);
    r.bg = colour == DVG_MOSAIC_RED ? q : colour == DVG_MOSAIC_GREEN ? q << 8 : 0u;
    r.label = (a.labels && label >= 0 && label < a.n_labels) ? a.labels + (size_t)label * a.lh * a.lw : nullptr;
    r.img = nullptr;
    // every index that comes from device memory is checked here: a bad table entry or index draws the background only
    long s = 0;
    bool ok = src >= 0 && src < 3;
    if (sel == DVG_MOSAIC_SEL_BEST) {
        ok = ok && a.best && b >= 0 && b < a.n_best;
        if (ok) s = a.best[b];
    } else if (sel == DVG_MOSAIC_SEL_PICK) {
        ok = ok && a.picks && b >= 0 && b < a.n_pick_rows && k >= 0 && k < a.pick_k;
        if (ok) s = a.picks[(size_t)b * a.pick_k + k];
    } else {
        ok = ok && sel == DVG_MOSAIC_SEL_NONE;
    }
    if (ok) {
        ok = s >= 0 && s < a.n_img[src];                        // also bounds the product below
        const long idx = (long)base + s * (long)stride;
        if (ok && a.src[src] && idx >= 0 && idx < a.n_img[src]) r.img = a.src[src] + (size_t)idx * a.nc * a.H * a.W;
    }
    return r;
}

// The three bytes of mosaic pixel (f, y, x), packed R | G << 8 | B << 16.  `key` / `cell` cache the cell of the previous pixel.
__device__ __forceinline__ unsigned mosaic_pixel(const MosaicArgs& a, unsigned f, unsigned y, unsigned x, unsigned& key,
                                                 MosaicCell& cell) {
    const unsigned ph = a.cell_h + a.pad_y, pw = a.cell_w + a.pad_x;
    const unsigned gy = y / ph, ry = y - gy * ph, gx = x / pw, rx = x - gx * pw;
    if (ry >= (unsigned)a.cell_h || rx >= (unsigned)a.cell_w) return 0xffffffu;   // image_tensor's canvas of ones
    const unsigned k = (f * a.R + gy) * a.Cc + gx;
    if (k != key) {
        cell = resolve_cell(a, f, gy, gx);
        key = k;
    }
    if (cell.label && ry < (unsigned)a.lh && rx < (unsigned)a.lw && cell.label[ry * a.lw + rx]) return 0u;
    const unsigned iy = ry - a.oy, ix = rx - a.ox;            // unsigned: one compare covers both sides
    if (!cell.img || iy >= (unsigned)a.H || ix >= (unsigned)a.W) return cell.bg;
    const float* p = cell.img + (size_t)iy * a.W + ix;
    const unsigned r = quant_byte(p[0], a.quant);
    if (a.nc == 1) return r * 0x010101u;
    const size_t plane = (size_t)a.H * a.W;
    return r | quant_byte(p[plane], a.quant) << 8 | quant_byte(p[2 * plane], a.quant) << 16;
}

// One thread = four consecutive pixels of the flat [F][GH][GW] mosaic = 12 bytes = three whole dwords (12 i is a multiple
// of four whatever GW is, so no store is narrower than a dword except in the last, partial group).  When the four pixels
// lie in one image row and the source address is 16-byte aligned, the row is read as one 16-byte load per channel.
__global__ __launch_bounds__(256) void frame_mosaic_kernel(MosaicArgs a, unsigned n_pix) {
    const unsigned n_grp = (n_pix + 3) / 4;
    const unsigned ph = a.cell_h + a.pad_y, pw = a.cell_w + a.pad_x;
    for (unsigned g = blockIdx.x * blockDim.x + threadIdx.x; g < n_grp; g += gridDim.x * blockDim.x) {
        const unsigned p0 = g * 4;
        const unsigned row = p0 / a.GW;
        unsigned x = p0 - row * a.GW, f = row / a.GH, y = row - f * a.GH;
        unsigned key = 0xffffffffu;
        MosaicCell cell;
        unsigned px[4];
        bool done = false;
        if (x + 3 < a.GW) {                                    // fast path: four pixels inside one image row
            const unsigned gy = y / ph, ry = y - gy * ph, gx = x / pw, rx = x - gx * pw;
            const unsigned iy = ry - a.oy, ix = rx - a.ox;
            if (ry < (unsigned)a.cell_h && rx < (unsigned)a.cell_w && iy < (unsigned)a.H && ix + 3 < (unsigned)a.W &&
                ix < (unsigned)a.W) {
                cell = resolve_cell(a, f, gy, gx);
                const float* p = cell.img ? cell.img + (size_t)iy * a.W + ix : nullptr;
                const bool lab = cell.label && ry < (unsigned)a.lh && rx < (unsigned)a.lw;   // any label pixel possible
                if (p && !lab && (reinterpret_cast<uintptr_t>(p) & 15u) == 0 &&(a.nc == 1 || (((size_t)a.H * a.W) & 3) == 0)) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p);
                    if (a.nc == 1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) px[j] = quant_byte(v0[j], a.quant) * 0x010101u;
                    } else {
                        const size_t plane = (size_t)a.H * a.W;
                        const f32x4 v1 = *reinterpret_cast<const f32x4*>(p + plane);
                        const f32x4 v2 = *reinterpret_cast<const f32x4*>(p + 2 * plane);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            px[j] = quant_byte(v0[j], a.quant) | quant_byte(v1[j], a.quant) << 8 |
                                    quant_byte(v2[j], a.quant) << 16;
                    }
                    done = true;
                }
            }
        }
        if (!done) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                px[j] = p0 + j < n_pix ? mosaic_pixel(a, f, y, x, key, cell) : 0u;
                if (++x == a.GW) {
                    x = 0;
                    if (++y == a.GH) {
                        y = 0;
                        ++f;
                    }
                }
            }
        }
        // 4 x RGB -> three dwords, little endian: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        const unsigned d0 = px[0] | px[1] << 24;
        const unsigned d1 = px[1] >> 8 | px[2] << 16;
        const unsigned d2 = px[2] >> 16 | px[3] << 8;
        if (p0 + 4 <= n_pix) {
            unsigned* o = reinterpret_cast<unsigned*>(a.out + (size_t)p0 * 3);
            o[0] = d0;
            o[1] = d1;
            o[2] = d2;
        } else {                                               // the last, partial group: its bytes one by one
            const unsigned d[3] = {d0, d1, d2};
            const unsigned nb = (n_pix - p0) * 3;
            for (unsigned i = 0; i < nb; ++i) a.out[(size_t)p0 * 3 + i] = (unsigned char)(d[i >> 2] >> ((i & 3) * 8));
        }
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_frame_mosaic(const float* src0, long n0, const float* src1, long n1, const float* src2, long n2, int nc,
                                int H, int W, const int* cells, int F, int R, int Cc, int cell_h, int cell_w, int pad_y,
                                int pad_x, int oy, int ox, const long* best, int n_best, const int* picks, int n_pick_rows,
                                int pick_k, const unsigned char* labels, int n_labels, int lh, int lw, int quant,
                                unsigned char* out, void* stream) {
    DVG_REQUIRE(cells && out, DVG_ERR_NULL, "dvg_frame_mosaic: NULL cell table or output");
    DVG_REQUIRE(src0 || src1 || src2, DVG_ERR_NULL, "dvg_frame_mosaic: no source");
    DVG_REQUIRE((src0 ? n0 > 0 : n0 == 0) && (src1 ? n1 > 0 : n1 == 0) && (src2 ? n2 > 0 : n2 == 0), DVG_ERR_SHAPE,
                "dvg_frame_mosaic: a source's image count must be > 0, and 0 for a NULL source");
    DVG_REQUIRE((nc == 1 || nc == 3) && H > 0 && W > 0, DVG_ERR_SHAPE, "dvg_frame_mosaic: nc must be 1 or 3, H, W > 0");
    DVG_REQUIRE(F > 0 && R > 0 && Cc > 0 && cell_h > 0 && cell_w > 0 && pad_y >= 0 && pad_x >= 0, DVG_ERR_SHAPE,
                "dvg_frame_mosaic: empty grid");
    DVG_REQUIRE(oy >= 0 && ox >= 0 && (long)oy + H <= cell_h && (long)ox + W <= cell_w, DVG_ERR_SHAPE,
                "dvg_frame_mosaic: a %dx%d image at (%d,%d) does not fit the %dx%d cell", H, W, oy, ox, cell_h, cell_w);
    DVG_REQUIRE(quant == DVG_QUANT_TRUNC || quant == DVG_QUANT_NEAREST, DVG_ERR_SHAPE, "dvg_frame_mosaic: quant %d", quant);
    DVG_REQUIRE(best ? n_best > 0 : n_best == 0, DVG_ERR_SHAPE, "dvg_frame_mosaic: best / n_best disagree");
    DVG_REQUIRE(picks ? (n_pick_rows > 0 && pick_k > 0) : (n_pick_rows == 0 && pick_k == 0), DVG_ERR_SHAPE,
                "dvg_frame_mosaic: picks / n_pick_rows / pick_k disagree");
    DVG_REQUIRE(labels ? (n_labels > 0 && lh > 0 && lw > 0 && lh <= cell_h && lw <= cell_w)
                       : (n_labels == 0 && lh == 0 && lw == 0),
                DVG_ERR_SHAPE, "dvg_frame_mosaic: label masks must be [n][lh <= cell_h][lw <= cell_w], or absent");
    const long GH = (long)R * cell_h + (long)(R - 1) * pad_y, GW = (long)Cc * cell_w + (long)(Cc - 1) * pad_x;
    // the kernel indexes pixels, rows and table entries with 32-bit unsigned arithmetic
    DVG_REQUIRE(GH < (1L << 31) && GW < (1L << 31) && (long)F * GH * GW + 4 < (1L << 31) &&
                    (long)F * R * Cc * DVG_MOSAIC_CELL_INTS < (1L << 31) && (long)cell_h + pad_y < (1L << 30) &&
                    (long)cell_w + pad_x < (1L << 30),
                DVG_ERR_SHAPE, "dvg_frame_mosaic: %d frames of %ldx%ld pixels exceed the 32-bit offsets of the kernel", F, GH, GW);
    DVG_REQUIRE((long)nc * H * W < (1L << 31) && (long)n_labels * lh * lw < (1L << 31), DVG_ERR_SHAPE,
                "dvg_frame_mosaic: image or label masks exceed 32-bit offsets");
    MosaicArgs a;
    a.src[0] = src0, a.src[1] = src1, a.src[2] = src2;
    a.n_img[0] = n0, a.n_img[1] = n1, a.n_img[2] = n2;
    a.cells = cells, a.best = best, a.picks = picks, a.labels = labels, a.out = out;
    a.nc = nc, a.H = H, a.W = W;
    a.F = F, a.R = R, a.Cc = Cc, a.cell_h = cell_h, a.cell_w = cell_w, a.pad_y = pad_y, a.pad_x = pad_x, a.oy = oy, a.ox = ox;
    a.n_best = n_best, a.n_pick_rows = n_pick_rows, a.pick_k = pick_k;
    a.n_labels = n_labels, a.lh = lh, a.lw = lw, a.quant = quant;
    a.GH = (unsigned)GH, a.GW = (unsigned)GW;
    const long n_pix = (long)F * GH * GW;
    // grid sized to the chip: 256 CUs x 8 workgroups of 256 threads, a grid-stride loop over the rest
    hipLaunchKernelGGL(frame_mosaic_kernel, dim3(grid_for((n_pix + 3) / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a,
                       (unsigned)n_pix);
    return check_launch("dvg_frame_mosaic");
}

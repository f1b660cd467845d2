// dvg_clip_gather_u8: a batch of clips out of a device-resident pool of decoded uint8 frames, as the float32
// (T,B,C,H,W) list-of-frames that utils.normalize_data yields (utils.py:86-95) from what the KTH / BAIR / UCF loaders
// return (data/kth.py:52-56 `imread(f)/255.` and `im[:, :, 0]`, data/bair.py:52-57, data/ucf.py:56-61).  HBM-bound: one
// byte read, four written.  Every lane loads 16 bytes (1 KiB per wave instruction), the tile goes through LDS once, and
// every lane leaves with whole float4s of ONE channel: the C = 3 de-interleave is a register shuffle of the 12 bytes of
// four pixels, and each store instruction of a wave writes 1 KiB contiguously.
#include "dvg_common.h"

namespace dvg {

constexpr int CLIP_TILE_PX = 1024;   // pixels per wave and tile: 64 lanes x 16 bytes x PC loads = PC KiB of LDS

// byte i of a run of little-endian dwords (i is a compile-time constant after unrolling: v_cvt_f32_ubyte<i & 3>)
template <int N>
__device__ __forceinline__ float clip_byte(const unsigned (&w)[N], int i) {
    return (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

// PC = channels of the pool (interleaved, as PNG decodes), C = channels written: C == PC, or C == 1 with PC == 3 (channel 0:
// KTH's three equal channels).  One wave per workgroup; tile = CLIP_TILE_PX pixels of one frame.
template <int PC, int C>
__global__ __launch_bounds__(64) void clip_gather_kernel(const unsigned char* __restrict__ pool,
                                                         const long* __restrict__ first, float* __restrict__ out,
                                                         long n_frames, int T, int B, unsigned HW, unsigned tiles_per_frame,
                                                         unsigned n_tiles) {
    __shared__ u32x4_t lds[PC * 64];
    const unsigned lane = threadIdx.x;
    const size_t frame_bytes = (size_t)HW * PC;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // uniform over the wave: barriers are safe
        const unsigned f = tile / tiles_per_frame;                            // output frame t * B + b
        const unsigned p0 = (tile - f * tiles_per_frame) * CLIP_TILE_PX;
        const unsigned t = f / B, b = f - t * B;
        long src = first[b];                                                   // device data: clamped, never trusted
        src = src < 0 ? 0 : (src > n_frames - T ? n_frames - T : src);
        const unsigned char* in = pool + (size_t)(src + t) * frame_bytes + (size_t)p0 * PC;   // 64-bit: pools exceed 4 GB
        const unsigned left = (HW - p0) * PC;                                  // bytes of this frame from the tile's start
#pragma unroll
        for (int j = 0; j < PC; ++j) {
            const unsigned off = (j * 64 + lane) * 16;
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (off < left) v = *reinterpret_cast<const u32x4_t*>(in + off);   // frame_bytes % 16 == 0: all 16 or none
            lds[j * 64 + lane] = v;
        }
        __syncthreads();
        const unsigned* words = reinterpret_cast<const unsigned*>(lds);
        float* o = out + (size_t)f * C * HW + p0;
#pragma unroll
        for (int i = 0; i < CLIP_TILE_PX / 4 / 64; ++i) {
            const unsigned q = i * 64 + lane;                                  // four consecutive pixels
            if (p0 + 4 * q < HW) {                                             // HW % 4 == 0: all four or none
                unsigned w[PC];
#pragma unroll
                for (int k = 0; k < PC; ++k) w[k] = words[q * PC + k];         // stride PC dwords per lane: no bank conflict
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    f32x4 r;
#pragma unroll
                    for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn(clip_byte(w, k * PC + c), 255.f);   // a division, not * (1/255)
                    *reinterpret_cast<f32x4*>(o + (size_t)c * HW + 4 * q) = r;
                }
            }
        }
        __syncthreads();
    }
}

// ---- dvg_clip_gather_aug_u8: the same gather with per-clip augmentation ------------------------------------------------------
// Per clip b: geom[b] = {hflip, reverse, dy, dx}, photo[b] = {gain, bias}.  A pure permutation of the decoded bytes (time
// reversal, horizontal flip, an integer shift with edge replication) followed by v -> clamp(gain * v + bias, 0, 1) as two
// separately rounded fp32 operations.  The reference's loaders have no augmentation: this extends data/kth.py:52-56,
// data/bair.py:52-57, data/ucf.py:56-61.  It moves exactly the bytes of the plain gather and keeps its global-memory shape:
// 16-byte loads, one trip through LDS, 1 KiB contiguous per store instruction of a wave.
//   * A tile is whole output ROWS (max(1, 1024 / W) of them, at most 1024 pixels), not a linear run of pixels: `reverse`,
//     `dy` and the row clamp then only decide WHICH source row a 16-byte load reads - whole aligned rows, nothing else.
//   * `hflip` and `dx` (with its column clamp) are applied when a lane reads its four pixels back out of LDS, byte by byte
//     (ds_read_u8, 4 x C per float4 group instead of the plain kernel's PC dword reads).  Consecutive lanes stand 4 pixels
//     = PC dwords apart, flipped or shifted alike, and PC in {1, 3} is coprime to the 32 banks: a 32-lane group reads 32
//     different banks, whatever dx is and in either direction; lanes that the column clamp sends to the same edge pixel read
//     the same dword, which is a broadcast.  A group that spans two rows can meet a 2-way conflict where the two rows' runs
//     of banks overlap.  A byte read costs an LDS cycle pair like a dword read; 12 of them per 3 KiB stored is an order of
//     magnitude below what the stores to HBM take, so the byte form was preferred to shuffling dwords under a branch.
// Nothing device-resident is trusted: first is clamped to [0, n_frames - T], dy / dx to +-DVG_CLIP_MAX_SHIFT, the source row
// and column to the frame, hflip / reverse are read as != 0; gain / bias never enter an address.
constexpr int DVG_CLIP_MAX_SHIFT = 16;

__device__ __forceinline__ int clip_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// n / d for n * d < 2^31 with m = ceil(2^31 / d) from the host: exact, since n * (m * d - 2^31) < n * d < 2^31
__device__ __forceinline__ unsigned clip_div(unsigned n, unsigned m) { return (unsigned)(((unsigned long)n * m) >> 31); }

// gain * v + bias as TWO fp32 roundings, what a float32 multiply followed by a float32 add gives on the host.  HIP compiles with
// -ffp-contract=fast, and its __fmul_rn / __fadd_rn are plain `*` and `+` in the header: inlined, they carry the contract flag
// and fuse into one FMA, an ulp away from the two roundings.  Under this pragma the two operations cannot fuse.
__device__ __forceinline__ float clip_mul_add(float gain, float v, float bias) {
#pragma clang fp contract(off)
    const float m = gain * v;
    return m + bias;
}

template <int PC, int C>
__global__ __launch_bounds__(64) void clip_gather_aug_kernel(const unsigned char* __restrict__ pool,
                                                             const long* __restrict__ first, const int* __restrict__ geom,
                                                             const float* __restrict__ photo, float* __restrict__ out,
                                                             long n_frames, int T, int B, int H, int W, unsigned rows_per_tile,
                                                             unsigned tiles_per_frame, unsigned n_tiles, unsigned m_cpr,
                                                             unsigned m_w4) {
    __shared__ u32x4_t lds[PC * 64];                                           // rows_per_tile * W <= 1024 pixels
    const unsigned lane = threadIdx.x;
    const unsigned HW = (unsigned)H * W;
    const unsigned row_bytes = (unsigned)W * PC;
    const unsigned cpr = row_bytes / 16, w4 = (unsigned)W / 4;                 // 16-byte chunks and float4 groups per row
    const size_t frame_bytes = (size_t)HW * PC;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // uniform over the wave: barriers are safe
        const unsigned f = tile / tiles_per_frame;                            // output frame t * B + b
        const unsigned y0 = (tile - f * tiles_per_frame) * rows_per_tile;
        const unsigned rows = min(rows_per_tile, (unsigned)H - y0);            // >= 1: tiles_per_frame = ceil(H / rows_per_tile)
        const unsigned t = f / B, b = f - t * B;
        long src = first[b];                                                   // device data: clamped, never trusted
        src = src < 0 ? 0 : (src > n_frames - T ? n_frames - T : src);
        const bool hflip = geom[4 * b] != 0, reverse = geom[4 * b + 1] != 0;
        const int dy = clip_clamp(geom[4 * b + 2], -DVG_CLIP_MAX_SHIFT, DVG_CLIP_MAX_SHIFT);
        const int dx = clip_clamp(geom[4 * b + 3], -DVG_CLIP_MAX_SHIFT, DVG_CLIP_MAX_SHIFT);
        const float gain = photo[2 * b], bias = photo[2 * b + 1];
        const unsigned ts = reverse ? (unsigned)T - 1 - t : t;                 // 0 <= ts < T
        const unsigned char* in = pool + (size_t)(src + ts) * frame_bytes;     // 64-bit: pools exceed 4 GB
#pragma unroll
        for (int j = 0; j < PC; ++j) {
            const unsigned k = j * 64 + lane;                                  // chunk k of the tile: row k / cpr, chunk k % cpr
            const unsigned r = clip_div(k, m_cpr);
            if (r < rows) {
                const unsigned sy = (unsigned)clip_clamp((int)(y0 + r) + dy, 0, H - 1);        // edge replicate
                lds[k] = *reinterpret_cast<const u32x4_t*>(in + (size_t)sy * row_bytes + (k - r * cpr) * 16);
            }
        }
        __syncthreads();
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(lds);
        float* o = out + (size_t)f * C * HW + (size_t)y0 * W;
#pragma unroll
        for (int i = 0; i < CLIP_TILE_PX / 4 / 64; ++i) {
            const unsigned q = i * 64 + lane;                                  // four consecutive pixels of one row (W % 4 == 0)
            const unsigned r = clip_div(q, m_w4);
            if (r < rows) {                                                    // only rows that were loaded are read
                const int x0 = (int)(q - r * w4) * 4;
                unsigned at[4];                                                // LDS byte offset of each source pixel
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int xs = hflip ? W - 1 - (x0 + k) : x0 + k;
                    at[k] = (r * (unsigned)W + (unsigned)clip_clamp(xs + dx, 0, W - 1)) * PC;
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    f32x4 v;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float u = __fdiv_rn((float)bytes[at[k] + c], 255.f);             // a division, not * (1/255)
                        v[k] = fminf(fmaxf(clip_mul_add(gain, u, bias), 0.f), 1.f);
                    }
                    *reinterpret_cast<f32x4*>(o + (size_t)c * HW + 4 * q) = v;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_clip_gather_u8(const uint8_t* pool, const int64_t* first, float* out, int64_t n_frames, int T, int B,
                                  int C, int H, int W, int pool_c, void* stream) {
    DVG_REQUIRE(pool && first && out, DVG_ERR_NULL, "dvg_clip_gather_u8: NULL pointer");
    DVG_REQUIRE(T >= 1 && B >= 1 && C >= 1 && H >= 1 && W >= 1, DVG_ERR_SHAPE, "dvg_clip_gather_u8: T, B, C, H, W must be >= 1");
    DVG_REQUIRE((pool_c == 1 || pool_c == 3) && (C == pool_c || (C == 1 && pool_c == 3)), DVG_ERR_SHAPE,
                "dvg_clip_gather_u8: C = %d from a pool of %d channels (C == pool_c in {1, 3}, or channel 0 of 3)", C, pool_c);
    DVG_REQUIRE(n_frames >= T, DVG_ERR_SHAPE, "dvg_clip_gather_u8: a pool of %ld frames holds no clip of %d", (long)n_frames, T);
    DVG_REQUIRE(((long)W * pool_c) % 16 == 0, DVG_ERR_SHAPE,
                "dvg_clip_gather_u8: rows of W * pool_c = %ld bytes are not a multiple of 16", (long)W * pool_c);
    DVG_REQUIRE((long)T * B * C * H * W < (1L << 31) && (long)H * W * pool_c < (1L << 31), DVG_ERR_SHAPE,
                "dvg_clip_gather_u8: %dx%dx%dx%dx%d output elements exceed the 32-bit offsets of the kernel", T, B, C, H, W);
    DVG_REQUIRE(aligned16(pool) && aligned16(out), DVG_ERR_ALIGN, "dvg_clip_gather_u8: pool / out not 16-byte aligned");
    const unsigned HW = (unsigned)H * W;
    const unsigned tpf = (HW + CLIP_TILE_PX - 1) / CLIP_TILE_PX;
    const long n_tiles = (long)T * B * tpf;
    DVG_REQUIRE(n_tiles < (1L << 31), DVG_ERR_SHAPE, "dvg_clip_gather_u8: too many tiles");
    // 256 CUs x 16 single-wave workgroups, a grid-stride loop over the rest
    const dim3 grid((unsigned)(n_tiles < 4096 ? n_tiles : 4096)), block(64);
    const long* fp = reinterpret_cast<const long*>(first);
    hipStream_t s = (hipStream_t)stream;
    if (pool_c == 1)
        hipLaunchKernelGGL((clip_gather_kernel<1, 1>), grid, block, 0, s, pool, fp, out, (long)n_frames, T, B, HW, tpf, (unsigned)n_tiles);
    else if (C == 1)
        hipLaunchKernelGGL((clip_gather_kernel<3, 1>), grid, block, 0, s, pool, fp, out, (long)n_frames, T, B, HW, tpf, (unsigned)n_tiles);
    else
        hipLaunchKernelGGL((clip_gather_kernel<3, 3>), grid, block, 0, s, pool, fp, out, (long)n_frames, T, B, HW, tpf, (unsigned)n_tiles);
    return check_launch("dvg_clip_gather_u8");
}

extern "C" int dvg_clip_gather_aug_u8(const uint8_t* pool, const int64_t* first, const int32_t* geom, const float* photo,
                                      float* out, int64_t n_frames, int T, int B, int C, int H, int W, int pool_c, void* stream) {
    DVG_REQUIRE(pool && first && out, DVG_ERR_NULL, "dvg_clip_gather_aug_u8: NULL pointer");
    DVG_REQUIRE(geom && photo, DVG_ERR_NULL, "dvg_clip_gather_aug_u8: NULL geom / photo");
    DVG_REQUIRE(T >= 1 && B >= 1 && C >= 1 && H >= 1 && W >= 1, DVG_ERR_SHAPE, "dvg_clip_gather_aug_u8: T, B, C, H, W must be >= 1");
    DVG_REQUIRE((pool_c == 1 || pool_c == 3) && (C == pool_c || (C == 1 && pool_c == 3)), DVG_ERR_SHAPE,
                "dvg_clip_gather_aug_u8: C = %d from a pool of %d channels (C == pool_c in {1, 3}, or channel 0 of 3)", C, pool_c);
    DVG_REQUIRE(n_frames >= T, DVG_ERR_SHAPE, "dvg_clip_gather_aug_u8: a pool of %ld frames holds no clip of %d", (long)n_frames, T);
    DVG_REQUIRE(((long)W * pool_c) % 16 == 0, DVG_ERR_SHAPE,
                "dvg_clip_gather_aug_u8: rows of W * pool_c = %ld bytes are not a multiple of 16", (long)W * pool_c);
    DVG_REQUIRE(W <= CLIP_TILE_PX, DVG_ERR_SHAPE, "dvg_clip_gather_aug_u8: W = %d exceeds the %d pixels of a tile", W, CLIP_TILE_PX);
    DVG_REQUIRE((long)T * B * C * H * W < (1L << 31) && (long)H * W * pool_c < (1L << 31), DVG_ERR_SHAPE,
                "dvg_clip_gather_aug_u8: %dx%dx%dx%dx%d output elements exceed the 32-bit offsets of the kernel", T, B, C, H, W);
    DVG_REQUIRE(aligned16(pool) && aligned16(out), DVG_ERR_ALIGN, "dvg_clip_gather_aug_u8: pool / out not 16-byte aligned");
    DVG_REQUIRE(aligned_to<4>(geom) && aligned_to<4>(photo), DVG_ERR_ALIGN,
                "dvg_clip_gather_aug_u8: geom / photo not 4-byte aligned");
    // W * pool_c % 16 == 0 with pool_c in {1, 3} makes W a multiple of 16: whole float4 groups and whole 16-byte chunks per row
    const unsigned rpt = (unsigned)(CLIP_TILE_PX / W);                         // >= 1: W <= CLIP_TILE_PX
    const unsigned tpf = ((unsigned)H + rpt - 1) / rpt;
    const long n_tiles = (long)T * B * tpf;
    DVG_REQUIRE(n_tiles < (1L << 31), DVG_ERR_SHAPE, "dvg_clip_gather_aug_u8: too many tiles");
    const unsigned cpr = (unsigned)((long)W * pool_c / 16), w4 = (unsigned)W / 4;
    const unsigned m_cpr = (unsigned)(((1UL << 31) + cpr - 1) / cpr), m_w4 = (unsigned)(((1UL << 31) + w4 - 1) / w4);   // clip_div
    const dim3 grid((unsigned)(n_tiles < 4096 ? n_tiles : 4096)), block(64);
    const long* fp = reinterpret_cast<const long*>(first);
    hipStream_t s = (hipStream_t)stream;
    if (pool_c == 1)
        hipLaunchKernelGGL((clip_gather_aug_kernel<1, 1>), grid, block, 0, s, pool, fp, geom, photo, out, (long)n_frames, T, B, H, W,
                           rpt, tpf, (unsigned)n_tiles, m_cpr, m_w4);
    else if (C == 1)
        hipLaunchKernelGGL((clip_gather_aug_kernel<3, 1>), grid, block, 0, s, pool, fp, geom, photo, out, (long)n_frames, T, B, H, W,
                           rpt, tpf, (unsigned)n_tiles, m_cpr, m_w4);
    else
        hipLaunchKernelGGL((clip_gather_aug_kernel<3, 3>), grid, block, 0, s, pool, fp, geom, photo, out, (long)n_frames, T, B, H, W,
                           rpt, tpf, (unsigned)n_tiles, m_cpr, m_w4);
    return check_launch("dvg_clip_gather_aug_u8");
}

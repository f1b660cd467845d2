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

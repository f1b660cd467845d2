// Moving-MNIST from real digits (data/moving_mnist.py), the device half.
//
// dvg_mnist_scale_u8: `transforms.Scale(32)` (moving_mnist.py:24-26) = Pillow's 8-bit bilinear resampler, bit for bit: a
// horizontal pass into a uint8 intermediate, then a vertical pass, each  clamp((2^21 + sum_k pixel * coef) >> 22, 0, 255)
// over the integer coefficients the host derives as Pillow does (dvg_amd/mnist.py).  Runs once per split; kept plain.
//
// dvg_moving_mnist_compose_u8: dvg_moving_mnist_compose (misc_kernels.hip) from the uint8 digit pool.  `ToTensor`'s
// float32 byte / 255 is a true division here (a multiply by 1/255 differs for 126 of the 256 bytes: clips.hip); the digits
// are added in index order and the sum is clipped at 1 (moving_mnist.py:86-90), written in normalize_data's layout.
#include "dvg_common.h"

namespace dvg {

constexpr int MNIST_DPW = 4;        // digits per workgroup of the scale kernel
constexpr int MNIST_MAX_SIZE = 64;  // largest out_size: 2 x 4 x 64 x 64 bytes of LDS
constexpr int MNIST_TAPS = 3;       // Pillow's ksize for an up-scaling bilinear filter; at most two are non-zero
constexpr int MNIST_PREC = 22;      // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ unsigned char mnist_clip8(int acc) {
    const int v = acc >> MNIST_PREC;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One pass over `line` (stride `step` bytes between taps): output position o of an axis of `in` input positions.
// xmin / coef are device data: the first tap is clamped into the line and taps past its end are skipped.
__device__ __forceinline__ unsigned char mnist_resample(const unsigned char* line, int step, int in, int o,
                                                        const int* __restrict__ xmin, const int* __restrict__ coef) {
    int x0 = xmin[o];
    x0 = x0 < 0 ? 0 : (x0 > in - 1 ? in - 1 : x0);
    int acc = 1 << (MNIST_PREC - 1);
#pragma unroll
    for (int k = 0; k < MNIST_TAPS; ++k)
        if (x0 + k < in) acc += (int)line[(x0 + k) * step] * coef[o * MNIST_TAPS + k];
    return mnist_clip8(acc);
}

__global__ __launch_bounds__(256) void mnist_scale_kernel(const unsigned char* __restrict__ raw,
                                                          unsigned char* __restrict__ out, int n, int in, int os,
                                                          const int* __restrict__ xmin, const int* __restrict__ coef) {
    extern __shared__ unsigned char lds[];
    unsigned char* src = lds;                              // [nd][in][in]
    unsigned char* mid = lds + MNIST_DPW * in * in;        // [nd][in][os]: the horizontal pass's uint8 result
    const int d0 = blockIdx.x * MNIST_DPW;
    const int nd = min(MNIST_DPW, n - d0);                 // the last workgroup may hold fewer digits
    const int tid = threadIdx.x;
    const unsigned char* g = raw + (size_t)d0 * in * in;
    for (int i = tid; i < nd * in * in; i += 256) src[i] = g[i];
    __syncthreads();
    for (int i = tid; i < nd * in * os; i += 256) {
        const int x = i % os, row = i / os;                // row = digit * in + y
        mid[i] = mnist_resample(src + row * in, 1, in, x, xmin, coef);
    }
    __syncthreads();
    unsigned char* o = out + (size_t)d0 * os * os;
    for (int i = tid; i < nd * os * os; i += 256) {
        const int x = i % os, y = (i / os) % os, d = i / (os * os);
        o[i] = mnist_resample(mid + d * in * os + x, os, in, y, xmin, coef);
    }
}

// One thread per four consecutive output pixels of a row (S % 4 == 0): one 16-byte store.
__global__ __launch_bounds__(256) void moving_mnist_compose_u8_kernel(const unsigned char* __restrict__ sprites,
                                                                      const int* __restrict__ ids, const int* __restrict__ pos,
                                                                      float* __restrict__ out, int T, int B, int ND, int S,
                                                                      int D, int n_sprites) {
    const int S4 = S >> 2;
    const long total = (long)T * B * S * S4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % S4) * 4;
        long r = i / S4;
        const int y = (int)(r % S); r /= S;
        const int b = (int)(r % B);
        const int t = (int)(r / B);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < ND; ++d) {                     // in digit order: three digits round as the host loop does
            const int* pp = pos + (((size_t)b * ND + d) * T + t) * 2;
            const int yy = y - pp[0], x0 = x - pp[1];
            if ((unsigned)yy >= (unsigned)D || x0 <= -4 || x0 >= D) continue;
            const unsigned char* row = sprites + ((size_t)min(max(ids[b * ND + d], 0), n_sprites - 1) * D + yy) * D;   // ids clamped: device data
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((unsigned)(x0 + k) < (unsigned)D) v[k] += __fdiv_rn((float)row[x0 + k], 255.f);   // a division, not * (1/255)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] > 1.f ? 1.f : v[k];
        *reinterpret_cast<f32x4*>(out + i * 4) = v;
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_mnist_scale_u8(const uint8_t* raw, uint8_t* out, int n, int in_size, int out_size, const int* xmin,
                                  const int* coef, void* stream) {
    DVG_REQUIRE(raw && out && xmin && coef, DVG_ERR_NULL, "dvg_mnist_scale_u8: NULL pointer");
    DVG_REQUIRE(n >= 1 && in_size >= 1, DVG_ERR_SHAPE, "dvg_mnist_scale_u8: n and in_size must be >= 1");
    DVG_REQUIRE(in_size <= out_size && out_size <= MNIST_MAX_SIZE, DVG_ERR_SHAPE,
                "dvg_mnist_scale_u8: %d -> %d: only up-scaling to at most %d is restated", in_size, out_size, MNIST_MAX_SIZE);
    const size_t lds = (size_t)MNIST_DPW * in_size * (in_size + out_size);
    hipLaunchKernelGGL(mnist_scale_kernel, dim3((unsigned)((n + MNIST_DPW - 1) / MNIST_DPW)), dim3(256), lds,
                       (hipStream_t)stream, raw, out, n, in_size, out_size, xmin, coef);
    return check_launch("dvg_mnist_scale_u8");
}

extern "C" int dvg_moving_mnist_compose_u8(const uint8_t* sprites, const int* ids, const int* pos, float* out, int n_sprites,
                                           int T, int B, int num_digits, int image_size, int digit_size, void* stream) {
    DVG_REQUIRE(sprites && ids && pos && out, DVG_ERR_NULL, "dvg_moving_mnist_compose_u8: NULL pointer");
    DVG_REQUIRE(n_sprites > 0 && T > 0 && B > 0 && num_digits > 0 && digit_size > 0 && image_size >= digit_size,
                DVG_ERR_SHAPE, "dvg_moving_mnist_compose_u8: bad shape");
    DVG_REQUIRE(image_size % 4 == 0, DVG_ERR_SHAPE, "dvg_moving_mnist_compose_u8: image_size %d is no multiple of 4", image_size);
    DVG_REQUIRE((long)n_sprites * digit_size * digit_size < (1L << 40), DVG_ERR_SHAPE, "dvg_moving_mnist_compose_u8: pool too large");
    DVG_REQUIRE(aligned16(out), DVG_ERR_ALIGN, "dvg_moving_mnist_compose_u8: out not 16-byte aligned");
    // ids / pos live in device memory: the kernel clamps ids and bounds-checks every sprite access against pos
    const long total = (long)T * B * image_size * (image_size / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(moving_mnist_compose_u8_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0,
                       (hipStream_t)stream, sprites, ids, pos, out, T, B, num_digits, image_size, digit_size, n_sprites);
    return check_launch("dvg_moving_mnist_compose_u8");
}

// Internal helpers shared by the kernel translation units of libdvg_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "../../include/dvg_hip.h"

namespace dvg {

// thread-local error string behind dvg_last_error()
char* err_buf();
int fail(int code, const char* fmt, ...);

template <unsigned N>
inline bool aligned_to(const void* p) {
    static_assert(N && !(N & (N - 1)), "a power of two");
    return (reinterpret_cast<uintptr_t>(p) & (N - 1)) == 0;      // NULL counts as aligned (optional pointers)
}
inline bool aligned16(const void* p) { return aligned_to<16>(p); }

// Workgroups for a grid-stride kernel over n items.  No default cap: the launchers do not agree on one (2048, 4096, 8192).
inline unsigned grid_for(long n, int block, int cap) {
    long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// Checks the launch that was just issued; no sync.
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DVG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return DVG_OK;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// ---- DVG_BF16X3: fp32 products on the bf16 matrix pipe ------------------------------------------------------------------
// gfx950's f32-input MFMA runs at 1/16 of the bf16 rate (157 vs 2516 TFLOP/s).  With DVG_BF16X3 = 1 the implicit-GEMM
// kernels (conv_igemm2.hip, wgrad.hip, wino_wgrad.hip) split every fp32 operand EXACTLY into three bf16 terms, a = h + m + l
// with 8 + 8 + 8 significant bits (h = a rounded to nearest bf16, m = the exact remainder a - h rounded to nearest bf16, l the
// rest: |m| <= 2^-8 |a|, |l| <= 2^-17 |a|, and l is a bf16 exactly), and form a K = 16 slab of the product as six
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation - (l,h) (m,m) (h,l) (m,h) (h,m) (h,h); bf16 x bf16 products are exact in
// fp32 and the dropped terms (m,l) (l,m) (l,l) are below 2^-24 |a||b| with no preferred sign, i.e. below the rounding of ONE
// fp32 product (tests/test_bf16x3_split.py restates this in numpy) - instead of eight v_mfma_f32_32x32x2_f32: 192 instead of
// 512 matrix-pipe cycles per slab.  Measured error against fp64: equal to or below the f32 MFMA's on every layer shape
// (tools/diag_mfma_precision.py, tests/test_gpu_parity.py).  The split is done ONCE per element: activations when a stage's
// tile is written to LDS, weights when they are packed (the packed row of 16 k-values is 3 x 16 bf16 = 24 floats).
// DVG_BF16X3 = 0 builds the native f32-MFMA library (same ABI; `dvg_mfma_mode()` tells which one is loaded).
#ifndef DVG_BF16X3
#define DVG_BF16X3 1
#endif
#define DVG_WROW (DVG_BF16X3 ? 24 : 16)   // floats per packed weight row (16 k-values of one output channel)

// two fp32 values -> their three bf16 terms, each pair packed into one dword (low half = the first value).  Nine VALU
// instructions: v_cvt_pk_bf16_f32 (round to nearest even) x 3, the two halves of a packed pair back to fp32 (shift / mask) x 2,
// v_pk_add_f32 x 2.  (A truncating split - mask instead of convert - costs the same and leaves dropped terms of up to
// 2^-20 |a||b|, all with the product's sign.)
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf16_pack_rn(float a0, float a1) {
    const f32x2_t v = {a0, a1};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ void bf16x3_split_pair(float a0, float a1, unsigned& ph, unsigned& pm, unsigned& pl) {
    const unsigned M = 0xffff0000u;
    const f32x2_t a = {a0, a1};
    ph = bf16_pack_rn(a0, a1);
    const f32x2_t h = {__uint_as_float(ph << 16), __uint_as_float(ph & M)};
    const f32x2_t r = a - h;
    pm = bf16_pack_rn(r[0], r[1]);
    const f32x2_t m = {__uint_as_float(pm << 16), __uint_as_float(pm & M)};
    const f32x2_t t = r - m;
    pl = bf16_pack_rn(t[0], t[1]);
}

// Packed weight rows.  A row = the 16 k-values (one 16-channel chunk) of ONE output channel; rows are stored in blocks of
// 64 output channels, [..][64][DVG_WROW], so that the weight tile of a workgroup's stage is one contiguous run.  With
// DVG_BF16X3 a row is [3 planes h, m, l][16 bf16], and the two 16-byte halves of every plane are swapped for rows with
// (co % 64) & 8 (the LDS image of the tile is this memory image: b128 fragment reads of 16 consecutive rows then hit 16
// distinct 16-byte slots).
// Two adjacent k-values (k even) of a packed row as ONE 4-byte store per plane (the r06 packed-row writer fix; the same values
// as 2 x 2-byte stores were equally clean: profiles/r06_dp_race_bisect.txt).
__device__ __forceinline__ void wrow_store_pair(float* __restrict__ rows, size_t row, int co_local, int k, float v0, float v1) {
#if DVG_BF16X3
    unsigned* d = reinterpret_cast<unsigned*>(rows + row * 24);
    unsigned ph, pm, pl;
    bf16x3_split_pair(v0, v1, ph, pm, pl);
    const int pos2 = ((((k >> 3) ^ ((co_local >> 3) & 1)) << 3) + (k & 7)) >> 1;
    d[pos2] = ph;
    d[8 + pos2] = pm;
    d[16 + pos2] = pl;
#else
    (void)co_local;
    rows[row * 16 + k] = v0;
    rows[row * 16 + k + 1] = v1;
#endif
}

// The last statement of every kernel that writes packed rows: the stores above performed before the wave ends (tried against the
// zero rows of winograd.hip's wrow_owner_note when they still looked like lost stores; harmless, kept - once per weight version).
__device__ __forceinline__ void wrow_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
    switch (act) {
        case DVG_ACT_LRELU: return v > 0.f ? v : v * slope;
        case DVG_ACT_TANH: return tanhf(v);
        case DVG_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        default: return v;
    }
}

// Bijective XCD-aware remap of a linear workgroup id (guide §5 T1): workgroups
// that land on one XCD (id % 8 equal) get a contiguous range of logical tiles.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7u, xcd = bid & 7u;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// ---- deterministic sums over a wave and over a workgroup ---------------------------------------------------------------------
// Every kernel that uses these promises the same bits on every launch, and saved training states, the --resume tests and the
// determinism tests compare bits: neither the tree inside a wave nor the order in which the wave sums are combined may change
// silently.  The two orders are historical, not chosen; each call site keeps the one it was written with.
//   SUM_WAVE_ORDER  ((0 + r0) + r1) + r2 ... left to right over the NT / 64 waves: gp.hip (gp_predict, gp_train_bwd, gp_elbo),
//                   grad_guard.hip (grad_sumsq, grad_guard_finish), ema.hip (ema_update), ssim_loss.hip (16 waves).  The leading + 0 is gp.hip's loop; the
//                   wave sums of grad_guard.hip and ema.hip are sums of squares from + 0, never - 0, so it changes none of their bits.
//                   validate.hip (val_accumulate) and gp_score.hip (gp_score): fp64 sums and int64 counts, four waves.
//   SUM_PAIRWISE    (r0 + r1) + (r2 + r3), four waves: finn_metrics.hip (eval_frames_finn) and eval_frames_kernel,
//                   frame_losses_kernel in misc_kernels.hip.
// One-wave kernels (gp_var_norms, gp_trigger_step, gp_trigger_replay) use wave_sum alone.

// The xor butterfly, offsets 32 ... 1: EVERY lane ends with the wave's sum.  Lane 0's value is also what the halving tree
// `v += __shfl_down(v, off)` leaves in lane 0 (grad_guard.hip and ema.hip were written with that one): at every level lane 0 adds
// its own value and lane `off`'s, and those two hold the same partial sums under either idiom - fp addition is commutative.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}

enum SumOrder { SUM_WAVE_ORDER, SUM_PAIRWISE };

// v[q] = the sum of v[q] over the workgroup's NT threads, for Q quantities under ONE pair of barriers; every thread gets the
// totals and every thread must call it.  `red`: Q * NT / 64 values of LDS.  The leading barrier lets a kernel call it again and
// again on the same `red` (a thread may still be reading the previous call's wave sums).
template <int NT, SumOrder ORDER = SUM_WAVE_ORDER, int Q, typename T>
__device__ __forceinline__ void block_sum(T (&v)[Q], T* red) {
    constexpr int NW = NT / 64;
    static_assert(NT % 64 == 0 && (ORDER == SUM_WAVE_ORDER || NW == 4), "whole waves; the pairwise order is written for four");
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) red[q * NW + (threadIdx.x >> 6)] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const T* r = red + q * NW;
        if constexpr (ORDER == SUM_PAIRWISE) {
            v[q] = (r[0] + r[1]) + (r[2] + r[3]);
        } else {
            T t = T(0.);
#pragma unroll
            for (int w = 0; w < NW; ++w) t += r[w];
            v[q] = t;
        }
    }
}

template <int NT, SumOrder ORDER = SUM_WAVE_ORDER, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    T a[1] = {v};
    block_sum<NT, ORDER>(a, red);
    return a[0];
}

}  // namespace dvg

#define DVG_REQUIRE(cond, code, ...) \
    do {                             \
        if (!(cond)) return dvg::fail(code, __VA_ARGS__); \
    } while (0)

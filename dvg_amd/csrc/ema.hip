// An exponential moving average of the flat parameter arena, kept ON THE DEVICE (train.py --ema_decay): the parameters are stepped
// through raw pointers inside a replayed hipGraph, so the average has to be a launch of that graph.  No reference counterpart: it
// follows the optimiser steps of the reference's train.py:242-245.  Semantics: docs/DESIGN_NOTES_ema.md.
//
//   dvg_ema_update   e' = fmaf(w, p - e, e) per element, w = (float)(1 - min(decay, (1 + k) / (10 + k))), k = *updates_dev;
//                    partials[2b] = sum (p - e')^2, partials[2b + 1] = sum p^2 over chunk b, fp64
//
// The weight is formed in fp64 INSIDE the kernel from the device-side count of updates already applied: a replayed graph gets a
// fresh weight at every replay.  The kernel only reads the count (no launch both reads and writes a counter); the caller advances
// it with a one-element add after the launch.  The update is an explicit fmaf, so its bits do not depend on the contraction mode,
// and its form keeps (1 - d) p when that is below an ulp of e (d e + (1 - d) p loses it at d = 0.9999).
//
// The two sums say how far the average lags the live weights: lag = sqrt(sum (p - e')^2) / sqrt(sum p^2), with e' the rounded value
// just stored.  Every term is formed in fp64 from the fp32 values (p^2 exactly; p - e' rounded once in fp64, its square added with
// an explicit fma), so an Inf or NaN in p reaches its own element of e and makes the lag sum of its chunk non-finite, nothing else.
//
// Order, as grad_sumsq_kernel: workgroup b owns the fixed chunk [b * EMA_CHUNK, (b + 1) * EMA_CHUNK) - no grid-stride loop, the
// number of partial pairs is a function of n alone (dvg_ema_update_blocks).  A thread adds its 16-byte pieces in index order into
// four fp64 sums per quantity (one per vector lane), those as (s0 + s1) + (s2 + s3), the 64 lanes of a wave and then the four
// waves through LDS in wave order by block_sum (dvg_common.h), both quantities under one pair of barriers.  No atomics: the
// same input gives the same bits on every launch.
//
// HBM-bound at 12 bytes per float (read p, read e, write e).  A thread issues all its loads of BOTH arrays - 2 x 8 x 16 bytes -
// before the first is consumed: 64 KiB per workgroup, the amount grad_sumsq_kernel keeps in flight.
#include "dvg_common.h"

namespace dvg {

constexpr int EMA_THREADS = 256;
constexpr int EMA_PIECES = 8;                                     // 16-byte loads per thread and array
constexpr long EMA_CHUNK = (long)EMA_THREADS * EMA_PIECES * 4;    // 8 192 floats per workgroup

// One workgroup's chunk.  FULL: every 16-byte piece of the chunk is inside the range - straight-line code, no index test.  Else
// (the last workgroup of a range that is no multiple of the chunk): a piece past the end is loaded from the last valid piece
// instead (never an address outside the range), counts as p = e = 0 - which adds nothing to either sum - and is not stored.
template <bool FULL>
__device__ __forceinline__ void ema_chunk(f32x4* __restrict__ e4, const f32x4* __restrict__ p4, long n4, float w, double& lag,
                                          double& sq) {
    const long base = (long)blockIdx.x * (EMA_CHUNK / 4) + threadIdx.x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 pv[EMA_PIECES], ev[EMA_PIECES];
#pragma unroll
    for (int j = 0; j < EMA_PIECES; ++j) {           // all loads of both arrays in flight before the first is consumed
        const long i = base + (long)j * EMA_THREADS;
        const long ic = FULL || i < n4 ? i : n4 - 1;
        pv[j] = p4[ic];
        ev[j] = e4[ic];
    }
    __builtin_amdgcn_sched_barrier(0);               // the scheduler would sink half of the loads below the first stores
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
    for (int j = 0; j < EMA_PIECES; ++j) {
        const long i = base + (long)j * EMA_THREADS;
        const bool in = FULL || i < n4;
        const f32x4 p = in ? pv[j] : zero, e = in ? ev[j] : zero;
        f32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = fmaf(w, p[c] - e[c], e[c]);
        if (in) e4[i] = o;
        const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2], p3 = (double)p[3];
        const double d0 = p0 - (double)o[0], d1 = p1 - (double)o[1], d2 = p2 - (double)o[2], d3 = p3 - (double)o[3];
        l0 = fma(d0, d0, l0);
        l1 = fma(d1, d1, l1);
        l2 = fma(d2, d2, l2);
        l3 = fma(d3, d3, l3);
        q0 = fma(p0, p0, q0);
        q1 = fma(p1, p1, q1);
        q2 = fma(p2, p2, q2);
        q3 = fma(p3, p3, q3);
    }
    lag = (l0 + l1) + (l2 + l3);
    sq = (q0 + q1) + (q2 + q3);
}

__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ param,
                                                                  long n4, double decay, const int* __restrict__ updates_dev,
                                                                  double* __restrict__ partials) {
    __shared__ double red[2 * 4];
    const double k = (double)*updates_dev;           // updates already applied; read, never written here
    const double warm = (1.0 + k) / (10.0 + k);
    const float w = (float)(1.0 - (decay < warm ? decay : warm));
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(param);
    double s[2];                                             // lag, sum of squares
    if (((long)blockIdx.x + 1) * (EMA_CHUNK / 4) <= n4)      // uniform over the workgroup
        ema_chunk<true>(e4, p4, n4, w, s[0], s[1]);
    else
        ema_chunk<false>(e4, p4, n4, w, s[0], s[1]);
    block_sum<EMA_THREADS>(s, red);
    if (threadIdx.x == 0) {
        partials[2 * (long)blockIdx.x] = s[0];
        partials[2 * (long)blockIdx.x + 1] = s[1];
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_ema_update_blocks(long n) {
    if (n <= 0) return 0;
    const long b = (n + EMA_CHUNK - 1) / EMA_CHUNK;
    return b > 0x3fffffffL ? 0 : (int)b;             // 2 b partial sums must be countable in an int as well
}

extern "C" int dvg_ema_update(float* ema, const float* param, long n, double decay, const int* updates_dev, double* partials,
                              void* stream) {
    DVG_REQUIRE(ema && param && updates_dev && partials, DVG_ERR_NULL, "dvg_ema_update: NULL pointer");
    DVG_REQUIRE(n > 0 && n % 4 == 0 && dvg_ema_update_blocks(n) > 0, DVG_ERR_SHAPE,
                "dvg_ema_update: n = %ld must be a positive multiple of 4", n);
    DVG_REQUIRE(decay >= 0.0 && decay < 1.0, DVG_ERR_SHAPE, "dvg_ema_update: decay = %g must be in [0, 1)", decay);   // NaN fails
    DVG_REQUIRE(aligned16(ema) && aligned16(param) && aligned_to<8>(partials) && aligned_to<4>(updates_dev), DVG_ERR_ALIGN,
                "dvg_ema_update: ema and param must be 16-byte, partials 8-byte, updates_dev 4-byte aligned");
    DVG_REQUIRE(ema != param, DVG_ERR_SHAPE, "dvg_ema_update: ema and param are the same buffer");
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)dvg_ema_update_blocks(n)), dim3(EMA_THREADS), 0, (hipStream_t)stream,
                       ema, param, n >> 2, decay, updates_dev, partials);
    return check_launch("dvg_ema_update");
}

// dvg_gp_score: the held-out scores of the GP trigger's predictive (train.py --val_gp, generate_frames.py --gp_report).  The GP's
// variance decides when a new future is triggered and its draw is that future (generate_frames.py:131,170,229 and train.py:283 read
// the predictive); this kernel reduces, per row r of an eval-mode predictive (mean, var: (R, B) fp32) and a target (R, B), what a
// probabilistic regressor is scored by: the negative log predictive density, the standardised residuals, the 68 % / 95 % coverage
// counts, the PIT deciles and the moments behind the variance ~ squared-error correlation.  The reference has no counterpart.
//
// Per entry (r, b), everything in fp64: v = var + noise[r % P] (noise NULL: v = var, the latent f), y = target, e = y - mean.  The
// entry is TAKEN if mean, var and y are finite and v > 0; otherwise it adds 1 to cnt[r][1] and nothing else.  A taken entry adds
//   acc[r][0..13] += 1/2 (ln 2 pi + ln v + e^2 / v), e, e^2, v, e / sqrt v, e^2 / v, y, y^2, v^2, e^4, v e^2, |e|, ln v, sqrt v
//   cnt[r][0] += 1;  cnt[r][2] += (e^2 <= v);  cnt[r][3] += (e^2 <= 3.84... v)        (the 68 % and 95 % intervals)
//   cnt[r][4 + k] += 1, k = #{ j : e |e| > c_j v }, c_j = the signed square of the standard normal's j-th decile edge (the PIT decile)
// Every count is decided by products and comparisons alone - no division, sqrt or erf - so that a numpy statement of the same two
// IEEE multiplications gives the same integers.
//
// Form.  One 256-thread workgroup per row r.  A thread takes b = tid, tid + 256, ... in ascending order and keeps 14 fp64 sums and 14
// counts of its own; the workgroup combines them with block_sum (the xor butterfly inside a wave, then the four wave sums left to
// right) and 14 + 14 threads each add one total to one output element.  The geometry is fixed - R workgroups of 256 - so the order
// of every sum is a function of (R, B) alone: no atomics, the same bits on every launch.  acc and cnt are ADDED to: K batches are
// K launches and one readback.
#include "dvg_common.h"

namespace dvg {

constexpr int GPS_NT = 256;
constexpr int GPS_ACC = 14;
constexpr int GPS_CNT = 14;

__device__ __forceinline__ bool gps_finite(double v) { return fabs(v) < __builtin_huge_val(); }   // false for NaN

__global__ __launch_bounds__(GPS_NT) void gp_score_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                          const float* __restrict__ noise, int period,
                                                          const float* __restrict__ target, long t_stride_r, long t_stride_b, int B,
                                                          double* __restrict__ acc, long long* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ double red_d[GPS_ACC * (GPS_NT / 64)];
    __shared__ long long red_n[GPS_CNT * (GPS_NT / 64)];
    constexpr double LN_2PI = 1.8378770664093453;
    constexpr double CHI2_95 = 3.8414588206941236;
    // the signed squares of the standard normal's quantiles at 0.1 ... 0.9
    constexpr double EDGE[9] = {-1.6423744151498172, -0.708326300800794, -0.2749958977284559, -0.06418475466730157, 0.0,
                                0.06418475466730157, 0.2749958977284559, 0.708326300800794,  1.6423744151498172};
    const int r = blockIdx.x;
    const double nz = noise != nullptr ? (double)noise[r % period] : 0.0;
    const float* mrow = mean + (size_t)r * B;
    const float* vrow = var + (size_t)r * B;
    const float* trow = target + (long)r * t_stride_r;
    double sums[GPS_ACC];
    long long counts[GPS_CNT];
#pragma unroll
    for (int q = 0; q < GPS_ACC; ++q) sums[q] = 0.0;
#pragma unroll
    for (int q = 0; q < GPS_CNT; ++q) counts[q] = 0;
    for (int b = threadIdx.x; b < B; b += GPS_NT) {
        const double m = (double)mrow[b], s = (double)vrow[b], y = (double)trow[(long)b * t_stride_b];
        const double v = s + nz;
        if (!(gps_finite(m) && gps_finite(s) && gps_finite(y) && v > 0.0)) {
            counts[1] += 1;
            continue;
        }
        const double e = y - m;
        const double e2 = e * e;
        const double ae = fabs(e);
        const double lv = log(v), sv = sqrt(v);
        const double q = e2 / v;
        sums[0] += 0.5 * ((LN_2PI + lv) + q);
        sums[1] += e;
        sums[2] += e2;
        sums[3] += v;
        sums[4] += e / sv;
        sums[5] += q;
        sums[6] += y;
        sums[7] += y * y;
        sums[8] += v * v;
        sums[9] += e2 * e2;
        sums[10] += v * e2;
        sums[11] += ae;
        sums[12] += lv;
        sums[13] += sv;
        counts[0] += 1;
        counts[2] += (e2 <= v) ? 1 : 0;
        counts[3] += (e2 <= CHI2_95 * v) ? 1 : 0;
        const double se = e * ae;
        int k = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) k += (se > EDGE[j] * v) ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 10; ++j) counts[4 + j] += (j == k) ? 1 : 0;      // (a register array is not indexed by a lane-dependent value)
    }
    block_sum<GPS_NT>(sums, red_d);
    block_sum<GPS_NT>(counts, red_n);
    // acc [R][14], cnt [R][14]: one thread per output element of this row
    const int t = threadIdx.x;
    if (t < GPS_ACC) {
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < GPS_ACC; ++k)
            if (k == t) total = sums[k];
        acc[(size_t)r * GPS_ACC + t] += total;
    } else if (t >= 64 && t < 64 + GPS_CNT) {
        long long total = 0;
#pragma unroll
        for (int k = 0; k < GPS_CNT; ++k)
            if (k == t - 64) total = counts[k];
        cnt[(size_t)r * GPS_CNT + (t - 64)] += total;
    }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_gp_score_slots(int* acc_slots, int* cnt_slots) {
    if (acc_slots) *acc_slots = GPS_ACC;
    if (cnt_slots) *cnt_slots = GPS_CNT;
    return DVG_OK;
}

extern "C" int dvg_gp_score(const float* mean, const float* var, const float* noise, int noise_period, const float* target,
                            long t_stride_r, long t_stride_b, int B, int R, double* acc, long long* cnt, void* stream) {
    DVG_REQUIRE(B >= 1 && R >= 1, DVG_ERR_SHAPE, "dvg_gp_score: B and R must be >= 1 (got %d, %d)", B, R);
    DVG_REQUIRE(noise_period >= 0 && R % (noise_period ? noise_period : R) == 0, DVG_ERR_SHAPE,
                "dvg_gp_score: the noise period %d must be >= 0 and divide R = %d", noise_period, R);
    DVG_REQUIRE(mean && var && target && acc && cnt, DVG_ERR_NULL, "dvg_gp_score: NULL pointer (only `noise` may be NULL)");
    hipLaunchKernelGGL(gp_score_kernel, dim3((unsigned)R), dim3(GPS_NT), 0, (hipStream_t)stream, mean, var, noise,
                       noise_period ? noise_period : R, target, t_stride_r, t_stride_b, B, acc, cnt);
    return check_launch("dvg_gp_score");
}

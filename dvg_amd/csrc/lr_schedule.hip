// The learning-rate multiplier of an iteration, kept ON THE DEVICE (train.py --lr_schedule): the Adam steps of an iteration are
// launches of a replayed hipGraph with their arguments baked in, so a rate that moves every iteration has to be read from device
// memory, like the step counts, the clip factor and the EMA weight.  No reference counterpart: its train.py hard-codes lr = 0.002
// (:95-104) and moves only the GP optimiser's, per epoch (:105-106).  Semantics: docs/DESIGN_NOTES_lr_schedule.md.
//
//   dvg_lr_schedule_tick   k = *iter_dev;  *scale_dev = (float)s(k);  *iter_dev = min(k + 1, INT_MAX)
//
// k counts the training iterations completed before this one - iterations whose step a gradient guard skipped included.  With
// W warm-up iterations, N iterations in all, the floor ratio R and, for `step`, the factor G every K iterations:
//
//   k < W      s = (k + 1) / W
//   else       u = min(1, (k - W) / max(1, N - W))
//     constant s = 1
//     linear   s = R + (1 - R) (1 - u)
//     cosine   s = R + (1 - R) (1/2 (1 + cos(pi u)))
//     step     s = max(R, G^floor((k - W) / K))
//
// in fp64, every operation rounded on its own (no contraction: the host restatement tests/lr_schedule_ref.py does the same
// operations in the same order, and agrees bit for bit wherever cos and pow are exact), rounded ONCE to fp32.  One thread of one
// workgroup: the launch is the whole cost.  Unlike dvg_ema_update this launch reads AND writes its counter: it is the only one that
// touches it, one thread does both, and the Adam launches that follow in stream order read only the scale.
#include <climits>

#include "dvg_common.h"

namespace dvg {

enum { LR_CONSTANT = 0, LR_LINEAR = 1, LR_COSINE = 2, LR_STEP = 3 };   // `kind`, as include/dvg_hip.h numbers them

__device__ __forceinline__ double lr_multiplier(int kind, int W, int N, int K, double R, double G, int k) {
#pragma clang fp contract(off)
    if (k < W) return ((double)k + 1.0) / (double)W;
    const int span = N - W > 1 ? N - W : 1;
    const double q = (double)(k - W) / (double)span, u = q < 1.0 ? q : 1.0;
    switch (kind) {
        case LR_LINEAR:
            return R + (1.0 - R) * (1.0 - u);
        case LR_COSINE:
            return R + (1.0 - R) * (0.5 * (1.0 + cos(M_PI * u)));
        case LR_STEP: {
            const double s = pow(G, (double)((k - W) / K));
            return s > R ? s : R;
        }
        default:
            return 1.0;
    }
}

__global__ void lr_schedule_tick_kernel(int kind, int W, int N, int K, double R, double G, int* __restrict__ iter_dev,
                                        float* __restrict__ scale_dev) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int k = *iter_dev;
    *scale_dev = (float)lr_multiplier(kind, W, N, K, R, G, k < 0 ? 0 : k);
    *iter_dev = k < INT_MAX ? k + 1 : INT_MAX;
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_lr_schedule_tick(int kind, int W, int N, int K, double R, double G, int* iter_dev, float* scale_dev,
                                    void* stream) {
    DVG_REQUIRE(iter_dev && scale_dev, DVG_ERR_NULL, "dvg_lr_schedule_tick: NULL pointer");
    DVG_REQUIRE(kind >= LR_CONSTANT && kind <= LR_STEP, DVG_ERR_SHAPE, "dvg_lr_schedule_tick: unknown kind %d", kind);
    DVG_REQUIRE(W >= 0 && N > W, DVG_ERR_SHAPE, "dvg_lr_schedule_tick: W = %d must be >= 0 and N = %d above it", W, N);
    DVG_REQUIRE(R >= 0.0 && R <= 1.0, DVG_ERR_SHAPE, "dvg_lr_schedule_tick: R = %g must be in [0, 1]", R);   // NaN fails
    DVG_REQUIRE(kind != LR_STEP || (K >= 1 && G > 0.0 && G <= 1.0), DVG_ERR_SHAPE,
                "dvg_lr_schedule_tick: step needs K = %d >= 1 and G = %g in (0, 1]", K, G);
    DVG_REQUIRE(aligned_to<4>(iter_dev) && aligned_to<4>(scale_dev), DVG_ERR_ALIGN,
                "dvg_lr_schedule_tick: iter_dev and scale_dev must be 4-byte aligned");
    hipLaunchKernelGGL(lr_schedule_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, kind, W, N, K, R, G, iter_dev, scale_dev);
    return check_launch("dvg_lr_schedule_tick");
}

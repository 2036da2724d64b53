// The Gaussian heat-map target of the hand-pose estimators' training (data/RHD_dataset.py:245-277), one definition for every
// kernel that needs it: mmh_heatmap_mse (hpe_train.hip) compares stage outputs with it, mmh_gauss_heatmaps (hpe3d_train.hip)
// writes it out as the 3D estimator's input.
#pragma once
#include <hip/hip_runtime.h>

namespace mmh {

// exp(-q) is below e^-5 = 0.0067 for q > 5: a third under the cut at 0.0099, against an error of the float64 exp near 1e-16.
// Such a target is 0 whatever exp would have returned, so leaving the call out cannot change a bit.
constexpr double HM_SKIP_Q = 5.0;

// t = (float)clip(exp(-D2 / 2.0 / sigma / sigma)), D2 = (ox - ux)^2 + (oy - uy)^2 in float64 without fused multiply-add; values
// above 1 -> 1, values below 0.0099 -> 0.  far2 = hm_far2(sigma): D2 beyond it means q > 5 whatever the two divisions round to
// (a relative 1e-6 against their 3e-16), so most pixels of a map are decided by one comparison and cost neither division nor
// exp; the q test behind it keeps the definition's own threshold for the rest.
__device__ __forceinline__ double hm_far2(double sigma) {
#pragma clang fp contract(off)
    return 2.0 * HM_SKIP_Q * sigma * sigma * 1.000001;
}

__device__ __forceinline__ float hm_target(double ox, double oy, double ux, double uy, double sigma, double far2) {
#pragma clang fp contract(off)
    const double dx = ox - ux, dy = oy - uy;
    const double d2 = dx * dx + dy * dy;
    if (d2 > far2) return 0.f;
    const double q = d2 / 2.0 / sigma / sigma;
    if (q > HM_SKIP_Q) return 0.f;
    double v = exp(-q);
    if (v > 1.0) v = 1.0;
    if (v < 0.0099) v = 0.0;
    return (float)v;
}

}  // namespace mmh

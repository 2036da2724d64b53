// The bilinear sampling rule of the passes that read uint8 images through a map (gfx950 only): the tap of the axis-aligned
// resize's callers (ResizeTap), the four-tap combination (lerp2) and the per-image inverse affine map of --augment_geom
// (affine_coord, affine_tap, affine_taps).  One definition for the decode passes (pointwise.hip) and the estimators'
// augmenting normalisation (hpe_augment.hip): a kernel file pulls them in with `using namespace mmh::dev;`.  Everything
// here is __forceinline__: one copy per translation unit.
#pragma once
#include "common.h"

namespace mmh { namespace dev {

struct ResizeTap { int i0, i1; double w; };

__device__ __forceinline__ double lerp2(double v00, double v01, double v10, double v11, double wx, double wy) {
    return (1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11);
}

// a = [a00 a01 a02; a10 a11 a12] takes the output pixel (x, y) to the source coordinate sx = (a00 x + a01 y) + a02,
// sy = (a10 x + a11 y) + a12.  Every product and sum is rounded on its own (contraction off), so the coordinates - and with
// them taps and weights - are numpy's bit for bit.  Edge replicate: the coordinate is clamped to [0, n - 1] BEFORE it becomes
// an integer; the comparisons are written so that a NaN lands on 0, and the integer is clamped once more, so no matrix
// whatever can index outside the image.
__device__ __forceinline__ void affine_coord(const double* __restrict__ a, int x, int y, double& sx, double& sy) {
#pragma clang fp contract(off)
    const double fx = (double)x, fy = (double)y;
    sx = (a[0] * fx + a[1] * fy) + a[2];
    sy = (a[3] * fx + a[4] * fy) + a[5];
}
__device__ __forceinline__ ResizeTap affine_tap(double s, int n_src) {
    const double hi = (double)(n_src - 1);
    s = s > 0.0 ? s : 0.0;                   // NaN compares false: 0
    s = s < hi ? s : hi;
    ResizeTap t;
    t.i0 = max(0, min((int)s, n_src - 1));   // 0 <= s <= n - 1: the cast is the floor
    t.i1 = min(t.i0 + 1, n_src - 1);
    t.w = s - (double)t.i0;
    return t;
}
// byte offsets of the four taps into one Hs x Ws x 3 uint8 image, and the two weights
struct AffineTaps { int64_t o00, o01, o10, o11; double wx, wy; };
__device__ __forceinline__ AffineTaps affine_taps(const double* __restrict__ a, int x, int y, int Hs, int Ws) {
    double sx, sy;
    affine_coord(a, x, y, sx, sy);
    const ResizeTap tx = affine_tap(sx, Ws), ty = affine_tap(sy, Hs);
    const int64_t row0 = (int64_t)ty.i0 * Ws, row1 = (int64_t)ty.i1 * Ws;
    AffineTaps t;
    t.o00 = (row0 + tx.i0) * 3, t.o01 = (row0 + tx.i1) * 3, t.o10 = (row1 + tx.i0) * 3, t.o11 = (row1 + tx.i1) * 3;
    t.wx = tx.w, t.wy = ty.w;
    return t;
}

}}  // namespace mmh::dev

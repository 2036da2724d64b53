// Depth condition of a 3D pose, rendered analytically for gfx950 (mmh_render_pose_depth; --depth_source joints, aug --novel):
// the 20 bones of the hand as capsules of `radius` pixels with a depth test, the stage the reference reaches with
// baselines/quantitative_on_benchmarks/utils.py:113-124,142-194 (joints (u, v, depth / 700 * 255) drawn bone by bone).
//
// Per pixel (x, y) and bone a -> b, all in float64 and every operation rounded on its own (contraction off, IEEE division):
//   dx = bu - au, dy = bv - av, L2 = dx dx + dy dy, px = x - au, py = y - av,
//   t = L2 > 0 ? (px dx + py dy) / L2 : 0, clamped to [0, 1] by two comparisons (a NaN stays a NaN and covers nothing),
//   cx = px - t dx, cy = py - t dy, covered iff cx cx + cy cy <= radius radius, z = az + t (bz - az).
// D = the smallest z of the covering bones, walked in the fixed bone order, or bg; stored ((D / 255) - 0.5) / 0.5 as fp32.
//
// One workgroup = one 32 x 8 pixel tile of one sample, both sides.  Lanes 0..19 and 32..51 of wave 0 each prepare one bone
// (the per-bone values dx, dy, dz, L2 are the per-pixel formula's own, computed once) and test its bounding box, grown by
// the radius and a margin, against the tile; the ballot of that test is the tile's bone list, kept in bone order.  The
// margin makes the cull invisible: a bone is culled only when all its coordinates are below 2^20 in magnitude, where the
// rounding of the per-pixel arithmetic is under 1e-8 pixels, while the box is grown by radius (1 + 1e-9) + 1e-3.  No
// atomics, nothing shared between workgroups; a thread owns its pixel's stores.
#include <cmath>
#include "common.h"

namespace {

constexpr int RTW = 32, RTH = 8;      // tile: a wave stores two rows of 32 pixels, 1 KB contiguous each in x_d
constexpr int RBONES = 20;
constexpr int RBF = 8;                // doubles per prepared bone: au av az dx dy dz L2 (+ 1 of padding)
constexpr double RCULL_MAX = 1048576.0;

// bone b of the order (0,1) (1,2) (2,3) (3,4) (0,5) (5,6) ... (19,20): four per finger, each finger starting at the wrist
__device__ __forceinline__ int bone_parent(int b) { return (b & 3) == 0 ? 0 : b; }

// out_lanes 8: x_d [N,H,W,8], side 0 -> lanes 0..2, side 1 -> lanes 3..5 (a NULL xyz leaves its lanes alone; both sides:
// two 16-byte stores, lanes 6 and 7 zero).  out_lanes 4: [N,H,W,4] from xyz0, lane 3 zero, one 16-byte store.
__global__ void __launch_bounds__(RTW * RTH) render_pose_depth_kernel(const double* __restrict__ xyz0, const double* __restrict__ xyz1,
                                                                       int H, int W, double radius, double bg,
                                                                       float* __restrict__ out, int out_lanes) {
#pragma clang fp contract(off)
    __shared__ double bone[2][RBONES][RBF];
    __shared__ unsigned long long hits;
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int x0 = blockIdx.x * RTW, y0 = blockIdx.y * RTH;
    if (tid < 64) {
        const int side = tid >> 5, b = tid & 31;
        const double* xyz = side == 0 ? xyz0 : xyz1;
        bool hit = false;
        if (b < RBONES && xyz != nullptr) {
            const double* pa = xyz + ((int64_t)n * 21 + bone_parent(b)) * 3;
            const double* pb = xyz + ((int64_t)n * 21 + b + 1) * 3;
            const double au = pa[0], av = pa[1], az = pa[2], bu = pb[0], bv = pb[1], bz = pb[2];
            const bool finite = __builtin_isfinite(au) && __builtin_isfinite(av) && __builtin_isfinite(az) &&
                                __builtin_isfinite(bu) && __builtin_isfinite(bv) && __builtin_isfinite(bz);
            if (finite) {
                const double dx = bu - au, dy = bv - av;
                double* s = bone[side][b];
                s[0] = au, s[1] = av, s[2] = az, s[3] = dx, s[4] = dy, s[5] = bz - az, s[6] = dx * dx + dy * dy;
                hit = true;
                const bool small = fabs(au) < RCULL_MAX && fabs(av) < RCULL_MAX && fabs(bu) < RCULL_MAX && fabs(bv) < RCULL_MAX;
                if (small) {
                    const double grow = radius * (1.0 + 1e-9) + 1e-3;
                    const double lo_u = fmin(au, bu) - grow, hi_u = fmax(au, bu) + grow;
                    const double lo_v = fmin(av, bv) - grow, hi_v = fmax(av, bv) + grow;
                    // written so that only a definite miss culls
                    if (hi_u < (double)x0 || lo_u > (double)(x0 + RTW - 1) || hi_v < (double)y0 || lo_v > (double)(y0 + RTH - 1))
                        hit = false;
                }
            }
        }
        const unsigned long long m = __ballot(hit);
        if (tid == 0) hits = m;
    }
    __syncthreads();
    const unsigned long long mask = hits;
    const int x = x0 + (tid & (RTW - 1)), y = y0 + (tid >> 5);
    if (x >= W || y >= H) return;
    const double r2 = radius * radius;
    const double fx = (double)x, fy = (double)y;
    float val[2] = {0.f, 0.f};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        unsigned m = (unsigned)(mask >> (32 * side)) & 0xFFFFFu;
        double D = bg;
        bool found = false;
        while (m) {
            const int b = __builtin_ctz(m);
            m &= m - 1;
            const double* s = bone[side][b];
            const double dx = s[3], dy = s[4], L2 = s[6];
            const double px = fx - s[0], py = fy - s[1];
            double t = L2 > 0.0 ? (px * dx + py * dy) / L2 : 0.0;
            t = t < 0.0 ? 0.0 : t;
            t = t > 1.0 ? 1.0 : t;
            const double cx = px - t * dx, cy = py - t * dy;
            const double d2 = cx * cx + cy * cy;
            const double z = s[2] + t * s[5];
            if (d2 <= r2 && (!found || z < D)) {
                D = z;
                found = true;
            }
        }
        val[side] = (float)(((D / 255.0) - 0.5) / 0.5);
    }
    const int64_t p = ((int64_t)n * H + y) * W + x;
    if (out_lanes == 4) {
        reinterpret_cast<float4*>(out)[p] = make_float4(val[0], val[0], val[0], 0.f);
    } else if (xyz0 != nullptr && xyz1 != nullptr) {
        float4* o = reinterpret_cast<float4*>(out) + p * 2;
        o[0] = make_float4(val[0], val[0], val[0], val[1]);
        o[1] = make_float4(val[1], val[1], 0.f, 0.f);
    } else {
        const int side = xyz0 != nullptr ? 0 : 1;
        float* o = out + p * 8 + 3 * side;
        o[0] = val[side], o[1] = val[side], o[2] = val[side];
    }
}

}  // namespace

int mmh_render_pose_depth(const double* xyz0, const double* xyz1, int N, int H, int W, double radius, double bg,
                          float* out, int out_lanes, mmh_stream_t s) {
    MMH_REQUIRE(out, "mmh_render_pose_depth: NULL output");
    MMH_REQUIRE(out_lanes == 4 || out_lanes == 8, "mmh_render_pose_depth: out_lanes = %d (4 = standalone, 8 = the decode passes' x_d)",
                out_lanes);
    MMH_REQUIRE(out_lanes == 8 ? (xyz0 || xyz1) : (xyz0 && !xyz1),
                "mmh_render_pose_depth: out_lanes 8 takes xyz0 and / or xyz1, out_lanes 4 takes xyz0 alone");
    MMH_REQUIRE(N > 0 && H > 0 && W > 0, "mmh_render_pose_depth: bad shape");
    MMH_REQUIRE(N <= 65535 && mmh::cdiv(H, RTH) <= 65535, "mmh_render_pose_depth: N = %d, H = %d exceed the launch grid", N, H);
    MMH_REQUIRE(radius >= 0.0 && std::isfinite(radius), "mmh_render_pose_depth: radius = %g (finite, >= 0)", radius);
    MMH_REQUIRE(std::isfinite(bg), "mmh_render_pose_depth: bg = %g (finite)", bg);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "mmh_render_pose_depth: the output must be 16-byte aligned");
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(xyz0) | reinterpret_cast<uintptr_t>(xyz1)) & 7) == 0,
                "mmh_render_pose_depth: xyz must be 8-byte aligned");
    hipLaunchKernelGGL(render_pose_depth_kernel, dim3((unsigned)mmh::cdiv(W, RTW), (unsigned)mmh::cdiv(H, RTH), (unsigned)N),
                       dim3(RTW * RTH), 0, mmh::as_stream(s), xyz0, xyz1, H, W, radius, bg, out, out_lanes);
    return mmh::check_launch("render_pose_depth");
}

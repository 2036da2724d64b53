// Training the 3D hand-pose estimator (mmhand_amd/hpe_train.py: Hpm3dTrainer), for gfx950: what the reference's recipe
// (hand_pose_estimators/CVPR2020_hpm3d/models/hpm3d_model.py:73,91-113) needs beside the convolutions' kernels.
//   * gauss_heatmaps: the network's input, the 21 Gaussian maps of RHD_dataset.py:245-277 at full resolution, written straight
//     into the 24-lane NHWC buffer conv1_1 reads.  One thread per (pixel, lane quad), one 16-byte store each; the value is
//     mmh::hm_target, the function mmh_heatmap_mse compares with.
//   * smooth_l1: nn.SmoothL1Loss() times a scale and its gradient, for the at most 64 x 24 outputs of depth_fc_3; one
//     workgroup, the terms added by one thread in ascending order.
//   * linear_dgrad, linear_wgrad: the backward of the depth head's nn.Linear layers.  VALU kernels of mmh_linear_fprop's
//     structure (operand tiles in LDS, a 4 x 4 register block per thread); every output element is one fp32 fma chain in a
//     fixed order, owned by one thread, so no atomics and no dependence on the grid.
#include <cmath>
#include "common.h"
#include "hpe_target.h"

namespace {

// ------------------------------------------------------------------------------------------------- the Gaussian maps
constexpr int GH_J = 21;
constexpr int GH_Q = 6;          // lane quads per pixel: 24 lanes
constexpr int GH_TPB = 256;

__global__ void __launch_bounds__(GH_TPB) gauss_heatmaps_kernel(const double* __restrict__ uv, int W, int64_t pixels, double sigma,
                                                                float* __restrict__ out, int cs) {
    __shared__ double suv[GH_J * 2];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < GH_J * 2) suv[tid] = uv[(int64_t)b * GH_J * 2 + tid];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * GH_TPB + tid;
    if (i >= pixels * GH_Q) return;
    const int64_t p = i / GH_Q;
    const int q = (int)(i - p * GH_Q);
    const double ox = (double)(p % W), oy = (double)(p / W);
    const double far2 = mmh::hm_far2(sigma);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = q * 4 + e;
        v[e] = j < GH_J ? mmh::hm_target(ox, oy, suv[2 * j], suv[2 * j + 1], sigma, far2) : 0.f;
    }
    *reinterpret_cast<float4*>(out + ((int64_t)b * pixels + p) * cs + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------------------------------------- smooth L1
constexpr int SL_MMAX = 64;
constexpr int SL_NMAX = 24;
constexpr int SL_TPB = 256;

__global__ void __launch_bounds__(SL_TPB) smooth_l1_kernel(const float* __restrict__ pred, int ps, const double* __restrict__ target,
                                                           int M, int n, double beta, double scale, double coef,
                                                           double* __restrict__ loss, float* __restrict__ dpred, int dcs) {
#pragma clang fp contract(off)
    __shared__ double terms[SL_MMAX * SL_NMAX];
    const int tid = threadIdx.x;
    for (int i = tid; i < M * (SL_NMAX / 4); i += SL_TPB) {
        const int m = i / (SL_NMAX / 4), q = i % (SL_NMAX / 4);
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = q * 4 + e;
            g[e] = 0.f;
            if (j < n) {
                const double d = (double)pred[(int64_t)m * ps + j] - target[m * n + j];
                const double a = fabs(d);
                const bool quad = a < beta;
                terms[m * n + j] = quad ? 0.5 * d * d / beta : a - 0.5 * beta;
                g[e] = (float)(coef * (quad ? d / beta : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0))));
            }
        }
        if (dpred) *reinterpret_cast<float4*>(dpred + (int64_t)m * dcs + q * 4) = make_float4(g[0], g[1], g[2], g[3]);
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < M * n; ++i) s = s + terms[i];
        loss[0] = scale * s / (double)(M * n);
    }
}

// ------------------------------------------------------------------------------------------------- nn.Linear backward
constexpr int LB_MMAX = 64;
constexpr int LB_T = 64;         // the tile of k (and, in wgrad, of n) per workgroup
constexpr int LB_NS = 32;        // columns of dy / wt per LDS step of dgrad
constexpr int LB_TPB = 256;      // 16 x 16 threads, a 4 x 4 block each
constexpr int LB_LD = LB_T + 4;  // row stride of the k-major tile: 16-byte rows

// dx[m][k] = sum_n dy[m][n] wt[k][n].  Workgroup = 64 rows k of wt x all m; thread (tc, tr): k = k0 + 4 tc .. + 3, m = tr + 16 r.
__global__ void __launch_bounds__(LB_TPB) linear_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ wt,
                                                              float* __restrict__ dx, int M, int K, int N) {
    __shared__ float dys[LB_MMAX][LB_NS + 1];
    __shared__ __attribute__((aligned(16))) float wts[LB_NS][LB_LD];        // [n][k]: transposed on the way in
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    const int k0 = blockIdx.x * LB_T;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int n0 = 0; n0 < N; n0 += LB_NS) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LB_MMAX * LB_NS / 4 / LB_TPB; ++j) {
            const int i = tid + j * LB_TPB, m = i / (LB_NS / 4), c4 = i % (LB_NS / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < M && n0 + c4 * 4 < N) v = *reinterpret_cast<const float4*>(dy + (int64_t)m * N + n0 + c4 * 4);
            dys[m][c4 * 4] = v.x; dys[m][c4 * 4 + 1] = v.y; dys[m][c4 * 4 + 2] = v.z; dys[m][c4 * 4 + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < LB_T * LB_NS / 4 / LB_TPB; ++j) {
            const int i = tid + j * LB_TPB, kk = i / (LB_NS / 4), c4 = i % (LB_NS / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + kk < K && n0 + c4 * 4 < N) v = *reinterpret_cast<const float4*>(wt + (int64_t)(k0 + kk) * N + n0 + c4 * 4);
            wts[c4 * 4][kk] = v.x; wts[c4 * 4 + 1][kk] = v.y; wts[c4 * 4 + 2][kk] = v.z; wts[c4 * 4 + 3][kk] = v.w;
        }
        __syncthreads();
        const int steps = min(LB_NS, N - n0);          // the zero-filled columns beyond N are not visited
        for (int nn = 0; nn < steps; ++nn) {
            const float4 wv = *reinterpret_cast<const float4*>(&wts[nn][tc * 4]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float g = dys[tr + 16 * r][nn];
                acc[r][0] = __builtin_fmaf(g, wv.x, acc[r][0]);
                acc[r][1] = __builtin_fmaf(g, wv.y, acc[r][1]);
                acc[r][2] = __builtin_fmaf(g, wv.z, acc[r][2]);
                acc[r][3] = __builtin_fmaf(g, wv.w, acc[r][3]);
            }
        }
    }
    const int k = k0 + tc * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = tr + 16 * r;
        if (m >= M) continue;
        float* o = dx + (int64_t)m * K + k;
        if ((K & 3) == 0) {                            // rows of dx are 16-byte aligned only then
            if (k < K) *reinterpret_cast<float4*>(o) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (k + c < K) o[c] = acc[r][c];
        }
    }
}

// dwt[k][n] = sum_m x[m][k] dy[m][n], db[n] = sum_m dy[m][n].  Workgroup = 64 k x 64 n with all M rows of both operands in LDS;
// thread (tc, tr): n = n0 + 4 tc .. + 3, k = k0 + 4 tr .. + 3.  The workgroups of the first k tile also write db.
__global__ void __launch_bounds__(LB_TPB) linear_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ dwt, float* __restrict__ db, int M, int K, int N) {
    __shared__ __attribute__((aligned(16))) float xs[LB_MMAX][LB_T];
    __shared__ __attribute__((aligned(16))) float dys[LB_MMAX][LB_T];
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    const int k0 = blockIdx.x * LB_T, n0 = blockIdx.y * LB_T;
    for (int i = tid; i < M * LB_T; i += LB_TPB) {
        const int m = i / LB_T, kk = i % LB_T;
        xs[m][kk] = k0 + kk < K ? x[(int64_t)m * K + k0 + kk] : 0.f;
    }
    for (int i = tid; i < M * (LB_T / 4); i += LB_TPB) {
        const int m = i / (LB_T / 4), c4 = i % (LB_T / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 + c4 * 4 < N) v = *reinterpret_cast<const float4*>(dy + (int64_t)m * N + n0 + c4 * 4);
        *reinterpret_cast<float4*>(&dys[m][c4 * 4]) = v;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int m = 0; m < M; ++m) {
        const float4 xv = *reinterpret_cast<const float4*>(&xs[m][tr * 4]);
        const float4 gv = *reinterpret_cast<const float4*>(&dys[m][tc * 4]);
        const float xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[r][0] = __builtin_fmaf(xr[r], gv.x, acc[r][0]);
            acc[r][1] = __builtin_fmaf(xr[r], gv.y, acc[r][1]);
            acc[r][2] = __builtin_fmaf(xr[r], gv.z, acc[r][2]);
            acc[r][3] = __builtin_fmaf(xr[r], gv.w, acc[r][3]);
        }
    }
    const int n = n0 + tc * 4;
    if (n < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + tr * 4 + r;
            if (k < K) *reinterpret_cast<float4*>(dwt + (int64_t)k * N + n) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        }
        if (db && blockIdx.x == 0 && tr == 0) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for (int m = 0; m < M; ++m) {
                const float4 gv = *reinterpret_cast<const float4*>(&dys[m][tc * 4]);
                s[0] = s[0] + gv.x; s[1] = s[1] + gv.y; s[2] = s[2] + gv.z; s[3] = s[3] + gv.w;
            }
            *reinterpret_cast<float4*>(db + n) = make_float4(s[0], s[1], s[2], s[3]);
        }
    }
}

bool lb_shape_ok(int M, int K, int N) {
    return M >= 1 && M <= LB_MMAX && K >= 1 && N >= 4 && N % 4 == 0 && (int64_t)K * N < (int64_t(1) << 40) &&
           mmh::cdiv(N, LB_T) <= 65535;
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

int mmh_gauss_heatmaps(const double* uv, int B, int H, int W, double sigma, float* out, int cs, mmh_stream_t s) {
    MMH_REQUIRE(uv && out, "mmh_gauss_heatmaps: NULL argument");
    MMH_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t(1) << 31) && cs >= 4 * GH_Q && cs % 4 == 0 &&
                    (int64_t)B * H * W * cs < (int64_t(1) << 40),
                "mmh_gauss_heatmaps: bad shape B=%d H=%d W=%d cs=%d (cs >= 24, cs %% 4 == 0)", B, H, W, cs);
    MMH_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "mmh_gauss_heatmaps: sigma must be positive and finite");
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(uv) & 7) == 0 && aligned16(out),
                "mmh_gauss_heatmaps: uv must be 8-byte and out 16-byte aligned");
    const int64_t pixels = (int64_t)H * W;
    hipLaunchKernelGGL(gauss_heatmaps_kernel, dim3((unsigned)mmh::cdiv(pixels * GH_Q, GH_TPB), B), dim3(GH_TPB), 0, mmh::as_stream(s),
                       uv, W, pixels, sigma, out, cs);
    return mmh::check_launch("gauss_heatmaps");
}

int mmh_smooth_l1(const float* pred, int ps, const double* target, int M, int n, double beta, double scale, double* loss,
                  float* dpred, int dcs, mmh_stream_t s) {
    MMH_REQUIRE(pred && target && loss, "mmh_smooth_l1: NULL argument");
    MMH_REQUIRE(M >= 1 && M <= SL_MMAX && n >= 1 && n <= SL_NMAX && ps >= n, "mmh_smooth_l1: bad shape M=%d n=%d ps=%d (M <= 64, n <= 24)",
                M, n, ps);
    MMH_REQUIRE(!dpred || (dcs >= SL_NMAX && dcs % 4 == 0), "mmh_smooth_l1: bad shape of the gradient, dcs=%d (dcs >= 24, dcs %% 4 == 0)",
                dcs);
    MMH_REQUIRE(beta > 0.0 && std::isfinite(beta), "mmh_smooth_l1: beta must be positive and finite");
    MMH_REQUIRE(std::isfinite(scale), "mmh_smooth_l1: scale is not finite");
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(loss)) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(pred) & 3) == 0 && aligned16(dpred),
                "mmh_smooth_l1: target and loss must be 8-byte, pred 4-byte and dpred 16-byte aligned");
    const double coef = scale / (double)(M * n);
    hipLaunchKernelGGL(smooth_l1_kernel, dim3(1), dim3(SL_TPB), 0, mmh::as_stream(s), pred, ps, target, M, n, beta, scale, coef, loss,
                       dpred, dcs);
    return mmh::check_launch("smooth_l1");
}

int mmh_linear_dgrad(const float* dy, const float* wt, float* dx, int M, int K, int N, mmh_stream_t s) {
    MMH_REQUIRE(dy && wt && dx, "mmh_linear_dgrad: NULL argument");
    MMH_REQUIRE(lb_shape_ok(M, K, N), "mmh_linear_dgrad: bad shape M=%d K=%d N=%d (M <= 64, N %% 4 == 0)", M, K, N);
    MMH_REQUIRE(aligned16(dy, wt, dx), "mmh_linear_dgrad: dy, wt and dx must be 16-byte aligned");
    hipLaunchKernelGGL(linear_dgrad_kernel, dim3((unsigned)mmh::cdiv(K, LB_T)), dim3(LB_TPB), 0, mmh::as_stream(s), dy, wt, dx, M, K, N);
    return mmh::check_launch("linear_dgrad");
}

int mmh_linear_wgrad(const float* x, const float* dy, float* dwt, float* db, int M, int K, int N, mmh_stream_t s) {
    MMH_REQUIRE(x && dy && dwt, "mmh_linear_wgrad: NULL argument");
    MMH_REQUIRE(lb_shape_ok(M, K, N), "mmh_linear_wgrad: bad shape M=%d K=%d N=%d (M <= 64, N %% 4 == 0)", M, K, N);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && aligned16(dy, dwt, db),
                "mmh_linear_wgrad: x must be 4-byte and dy, dwt and db 16-byte aligned");
    hipLaunchKernelGGL(linear_wgrad_kernel, dim3((unsigned)mmh::cdiv(K, LB_T), (unsigned)mmh::cdiv(N, LB_T)), dim3(LB_TPB), 0,
                       mmh::as_stream(s), x, dy, dwt, db, M, K, N);
    return mmh::check_launch("linear_wgrad");
}

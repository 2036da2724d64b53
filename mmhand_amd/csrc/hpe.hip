// The hand-pose estimators' passes around their convolutions (PCK evaluation, baselines/quantitative_on_benchmarks/
// hpe_estimator.py:97-143), for gfx950:
//   * hpe_normalize: cv2.normalize(NORM_MINMAX, alpha 1) of an image (RHD_dataset.py:121,215-227) into the estimator's NHWC
//     input.  Minimum and maximum are exact whatever the order they are taken in; the partials of an image are still
//     merged in a fixed order and there is no atomic.  (x - min) / (max - min) in float64, one rounding at the store.
//   * heatmap_upsample_argmax: nn.Upsample(scale_factor=8, bilinear, align_corners=True) of the heat maps (net_hpm2d.py:69,118)
//     and torch.max per joint (hpe_estimator.py:127-135) in one pass: a workgroup writes a band of output rows and the band's
//     (maximum, first index) per joint; a second kernel merges an image's bands in scan order.
//   * linear_fprop: the depth head's nn.Linear layers (net_hpm3d.py:60-62,110-114) for a handful of rows.  The contraction is
//     cut into chunks of LIN_KC rows of W.  A chunk's sum is one fma chain in k order, and the chunks are summed by
//     slab_reduce.hip in an order that depends on their number (and on the library option "slab_reduce_par", which picks
//     its kernel) - never on the grid of this kernel.
#include <cmath>
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------- normalise
constexpr int NRM_TPB = 256;
constexpr int NRM_MAX_CHUNKS = 64;

__host__ __device__ inline int nrm_chunks(int H, int W) {
    const int64_t px = (int64_t)H * W;
    const int64_t c = (px + NRM_TPB - 1) / NRM_TPB;
    return (int)(c < NRM_MAX_CHUNKS ? c : NRM_MAX_CHUNKS);
}

template <typename T>
__device__ __forceinline__ float px_at(const mmh_image_src& s, int64_t base, int c, int y, int x) {
    return (float)reinterpret_cast<const T*>(s.ptr)[base + (int64_t)c * s.sc + (int64_t)y * s.sh + (int64_t)x * s.sw];
}

// chunk `blockIdx.x` of image `blockIdx.y`: pixels chunk, chunk + chunks, ... (all three channels) -> part[b][chunk] = (min, max)
template <typename T>
__global__ void __launch_bounds__(NRM_TPB) hpe_minmax_kernel(mmh_image_src src, int H, int W, int chunks,
                                                             float2* __restrict__ part) {
    __shared__ float2 red[NRM_TPB];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int64_t base = (int64_t)b * src.sb, npx = (int64_t)H * W;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t p = (int64_t)chunk * NRM_TPB + tid; p < npx; p += (int64_t)chunks * NRM_TPB) {
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = px_at<T>(src, base, c, y, x);
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    red[tid] = make_float2(mn, mx);
    __syncthreads();
    for (int h = NRM_TPB / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = make_float2(fminf(red[tid].x, red[tid + h].x), fmaxf(red[tid].y, red[tid + h].y));
        __syncthreads();
    }
    if (tid == 0) part[(int64_t)b * chunks + chunk] = red[0];
}

// every workgroup of image b folds the image's partials (at most 64, in order) and normalises its own pixels
template <typename T>
__global__ void __launch_bounds__(NRM_TPB) hpe_normalize_kernel(mmh_image_src src, int H, int W, int chunks,
                                                                const float2* __restrict__ part, float4* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < chunks; ++i) {
        const float2 t = part[(int64_t)b * chunks + i];
        mn = fminf(mn, t.x);
        mx = fmaxf(mx, t.y);
    }
    const int64_t base = (int64_t)b * src.sb, npx = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * NRM_TPB + threadIdx.x;
    if (p >= npx) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const double lo = (double)mn, range = (double)mx - (double)mn;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        v[c] = range > 0.0 ? (float)(((double)px_at<T>(src, base, c, y, x) - lo) / range) : 0.f;
    out[(int64_t)b * npx + p] = make_float4(v[0], v[1], v[2], 0.f);
}

template <typename T>
int launch_normalize(const mmh_image_src& src, int B, int H, int W, float2* part, float4* out, hipStream_t st) {
    const int chunks = nrm_chunks(H, W);
    hipLaunchKernelGGL(hpe_minmax_kernel<T>, dim3(chunks, B), dim3(NRM_TPB), 0, st, src, H, W, chunks, part);
    if (int rc = mmh::check_launch("hpe_minmax")) return rc;
    hipLaunchKernelGGL(hpe_normalize_kernel<T>, dim3((unsigned)mmh::cdiv((int64_t)H * W, NRM_TPB), B), dim3(NRM_TPB), 0, st, src,
                       H, W, chunks, part, out);
    return mmh::check_launch("hpe_normalize");
}

// ------------------------------------------------------------------------------------------------- upsample + arg-max
constexpr int UP = 8;            // nn.Upsample(scale_factor=8)
constexpr int UP_J = 21;         // joints
constexpr int UP_C = 24;         // output lanes: 21 joints + 3 zeros
constexpr int UP_Q = UP_C / 4;   // float4 lanes per output pixel
constexpr int UP_PX = 32;        // output pixels a workgroup visits at a time
constexpr int UP_TPB = UP_PX * UP_Q;
constexpr int UP_ROWS = 8;       // output rows per workgroup
constexpr int UP_NONE = 0x7fffffff;

struct UpBest { float v; int idx; };

struct UpTap { int i0, i1; double w; };
// align_corners=True: source coordinate = o * (n_src - 1) / (n_out - 1), the ratio taken first (as ATen does), no fma
__device__ __forceinline__ UpTap up_tap(int o, int n_src, int n_out) {
#pragma clang fp contract(off)
    const double scale = n_out > 1 ? (double)(n_src - 1) / (double)(n_out - 1) : 0.0;
    const double s = scale * (double)o;
    UpTap t;
    t.i0 = min((int)s, n_src - 1);
    t.i1 = min(t.i0 + 1, n_src - 1);
    t.w = s - (double)t.i0;
    return t;
}
__device__ __forceinline__ float up_lerp(double v00, double v01, double v10, double v11, double wx, double wy) {
#pragma clang fp contract(off)
    return (float)((1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11));
}

// band blockIdx.x (UP_ROWS output rows) of image blockIdx.y.  Thread (pixel slot, q) owns lanes 4 q .. 4 q + 3 of the pixels
// slot, slot + 32, ... of the band, in scan order: a strictly greater value replaces its best, so the first one stays.
__global__ void __launch_bounds__(UP_TPB) hpe_upsample_kernel(const float* __restrict__ heat, int h, int w, int cs,
                                                              float4* __restrict__ up, UpBest* __restrict__ part) {
    __shared__ UpBest best_s[UP_TPB][4];
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const int Ho = h * UP, Wo = w * UP;
    const int q = tid % UP_Q, slot = tid / UP_Q;
    const int r0 = band * UP_ROWS;
    const int npx = min(UP_ROWS, Ho - r0) * Wo;
    const float* hb = heat + (int64_t)b * h * w * cs;
    UpBest best[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) best[e] = UpBest{-INFINITY, UP_NONE};
    for (int p = slot; p < npx; p += UP_PX) {
        const int oy = r0 + p / Wo, ox = p % Wo;
        const UpTap ty = up_tap(oy, h, Ho), tx = up_tap(ox, w, Wo);
        const float* p00 = hb + ((int64_t)ty.i0 * w + tx.i0) * cs;
        const float* p01 = hb + ((int64_t)ty.i0 * w + tx.i1) * cs;
        const float* p10 = hb + ((int64_t)ty.i1 * w + tx.i0) * cs;
        const float* p11 = hb + ((int64_t)ty.i1 * w + tx.i1) * cs;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = q * 4 + e;
            v[e] = 0.f;
            if (c < UP_J) {
                v[e] = up_lerp((double)p00[c], (double)p01[c], (double)p10[c], (double)p11[c], tx.w, ty.w);
                if (v[e] > best[e].v) best[e] = UpBest{v[e], oy * Wo + ox};
            }
        }
        up[((int64_t)b * Ho * Wo + (int64_t)oy * Wo + ox) * UP_Q + q] = make_float4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) best_s[tid][e] = best[e];
    __syncthreads();
    if (tid < UP_J) {
        const int jq = tid / 4, je = tid % 4;
        UpBest r = UpBest{-INFINITY, UP_NONE};
        for (int s = 0; s < UP_PX; ++s) {
            const UpBest t = best_s[s * UP_Q + jq][je];
            if (t.v > r.v || (t.v == r.v && t.idx < r.idx)) r = t;
        }
        part[((int64_t)b * gridDim.x + band) * UP_J + tid] = r;
    }
}

// an image's bands in scan order: a later band wins only with a strictly greater value
__global__ void __launch_bounds__(64) hpe_argmax_merge_kernel(const UpBest* __restrict__ part, int bands, int Wo,
                                                              int* __restrict__ arg, float* __restrict__ maxv) {
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= UP_J) return;
    UpBest r = UpBest{-INFINITY, UP_NONE};
    for (int t = 0; t < bands; ++t) {
        const UpBest c = part[((int64_t)b * bands + t) * UP_J + j];
        if (c.v > r.v || (c.v == r.v && c.idx < r.idx)) r = c;
    }
    const int idx = r.idx == UP_NONE ? 0 : r.idx;      // a map without a single comparable value (all NaN): pixel 0
    arg[((int64_t)b * UP_J + j) * 2 + 0] = idx % Wo;
    arg[((int64_t)b * UP_J + j) * 2 + 1] = idx / Wo;
    maxv[(int64_t)b * UP_J + j] = r.v;
}

int up_bands(int h) { return (int)mmh::cdiv((int64_t)h * UP, UP_ROWS); }

bool up_shape_ok(int B, int h, int w, int cs) {
    return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && cs >= UP_J && (int64_t)h * UP * w * UP < (int64_t(1) << 31) &&
           (int64_t)B * h * w * cs < (int64_t(1) << 40) && up_bands(h) <= 0x7fffffff;
}

// ------------------------------------------------------------------------------------------------- linear
constexpr int LIN_KC = 256;      // rows of W per chunk: the unit of the summation's definition
constexpr int LIN_KS = 32;       // rows of W per LDS step
constexpr int LIN_BN = 64;       // columns per workgroup
constexpr int LIN_MMAX = 64;
constexpr int LIN_TPB = 256;     // 16 column quads x 16 row groups of 4 rows

// workgroup (column tile blockIdx.x, split blockIdx.y) computes the chunks [split * cps, (split + 1) * cps) of its 64 columns,
// each into its own slab: slab[chunk][m][n] = (chunk == 0 ? bias[n] : 0) + sum over the chunk's k, ascending, one fma each
__global__ void __launch_bounds__(LIN_TPB) hpe_linear_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                             const float* __restrict__ bias, int M, int K, int N,
                                                             int chunks, int cps, float* __restrict__ slab) {
    __shared__ float xs[LIN_MMAX][LIN_KS + 1];
    __shared__ __attribute__((aligned(16))) float ws[LIN_KS][LIN_BN];
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    const int n0 = blockIdx.x * LIN_BN, col = n0 + tc * 4;
    const int c_end = min(chunks, ((int)blockIdx.y + 1) * cps);
    for (int chunk = blockIdx.y * cps; chunk < c_end; ++chunk) {
        float acc[4][4];
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (chunk == 0 && bias && col < N) bv = *reinterpret_cast<const float4*>(bias + col);
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[r][0] = bv.x; acc[r][1] = bv.y; acc[r][2] = bv.z; acc[r][3] = bv.w; }
        const int k_lo = chunk * LIN_KC, k_hi = min(K, k_lo + LIN_KC);
        for (int k0 = k_lo; k0 < k_hi; k0 += LIN_KS) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LIN_MMAX * LIN_KS / LIN_TPB; ++j) {
                const int i = tid + j * LIN_TPB, m = i / LIN_KS, kk = i % LIN_KS;
                xs[m][kk] = (m < M && k0 + kk < k_hi) ? x[(int64_t)m * K + k0 + kk] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < LIN_KS * LIN_BN / 4 / LIN_TPB; ++j) {
                const int i = tid + j * LIN_TPB, kk = i / (LIN_BN / 4), c4 = i % (LIN_BN / 4);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + kk < k_hi && n0 + c4 * 4 < N) v = *reinterpret_cast<const float4*>(wt + (int64_t)(k0 + kk) * N + n0 + c4 * 4);
                *reinterpret_cast<float4*>(&ws[kk][c4 * 4]) = v;
            }
            __syncthreads();
            const int steps = min(LIN_KS, k_hi - k0);      // the zero-filled rows beyond k_hi are not visited
            for (int kk = 0; kk < steps; ++kk) {
                const float4 wv = *reinterpret_cast<const float4*>(&ws[kk][tc * 4]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float xv = xs[tr + 16 * r][kk];
                    acc[r][0] = __builtin_fmaf(xv, wv.x, acc[r][0]);
                    acc[r][1] = __builtin_fmaf(xv, wv.y, acc[r][1]);
                    acc[r][2] = __builtin_fmaf(xv, wv.z, acc[r][2]);
                    acc[r][3] = __builtin_fmaf(xv, wv.w, acc[r][3]);
                }
            }
        }
        if (col < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = tr + 16 * r;
                if (m < M)
                    *reinterpret_cast<float4*>(slab + ((int64_t)chunk * M + m) * N + col) =
                        make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
            }
        }
    }
}

bool lin_shape_ok(int M, int K, int N) {
    return M >= 1 && M <= LIN_MMAX && K >= 1 && N >= 4 && N % 4 == 0 && (int64_t)K * N < (int64_t(1) << 40) &&
           mmh::cdiv(K, LIN_KC) <= 65535;
}

}  // namespace

size_t mmh_hpe_normalize_ws_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W >= (int64_t(1) << 31)) return 0;
    return (size_t)B * nrm_chunks(H, W) * sizeof(float2);
}

int mmh_hpe_normalize(const mmh_image_src* src, int B, int H, int W, void* ws, size_t ws_bytes, float* out, mmh_stream_t s) {
    MMH_REQUIRE(src && src->ptr && ws && out, "mmh_hpe_normalize: NULL argument");
    const size_t need = mmh_hpe_normalize_ws_bytes(B, H, W);
    MMH_REQUIRE(need > 0, "mmh_hpe_normalize: bad shape B=%d H=%d W=%d", B, H, W);
    MMH_REQUIRE(ws_bytes >= need, "mmh_hpe_normalize: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "mmh_hpe_normalize: out must be 16-byte and ws 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    float2* part = static_cast<float2*>(ws);
    float4* o = reinterpret_cast<float4*>(out);
    switch (src->dtype) {
        case MMH_F32: return launch_normalize<float>(*src, B, H, W, part, o, st);
        case MMH_BF16: return launch_normalize<__bf16>(*src, B, H, W, part, o, st);
        case MMH_FP16: return launch_normalize<_Float16>(*src, B, H, W, part, o, st);
        case MMH_U8: return launch_normalize<uint8_t>(*src, B, H, W, part, o, st);
        default: return mmh::fail("mmh_hpe_normalize: unknown dtype %d", src->dtype);
    }
}

size_t mmh_heatmap_upsample_argmax_ws_bytes(int B, int h, int w) {
    if (!up_shape_ok(B, h, w, UP_J)) return 0;
    return (size_t)B * up_bands(h) * UP_J * sizeof(UpBest);
}

int mmh_heatmap_upsample_argmax(const float* heat, int B, int h, int w, int cs, float* up, int32_t* arg, float* maxv, void* ws,
                                size_t ws_bytes, mmh_stream_t s) {
    MMH_REQUIRE(heat && up && arg && maxv && ws, "mmh_heatmap_upsample_argmax: NULL argument");
    MMH_REQUIRE(up_shape_ok(B, h, w, cs), "mmh_heatmap_upsample_argmax: bad shape B=%d h=%d w=%d cs=%d (cs >= 21)", B, h, w, cs);
    const size_t need = mmh_heatmap_upsample_argmax_ws_bytes(B, h, w);
    MMH_REQUIRE(ws_bytes >= need, "mmh_heatmap_upsample_argmax: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(up) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "mmh_heatmap_upsample_argmax: up must be 16-byte and ws 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    const int bands = up_bands(h);
    UpBest* part = static_cast<UpBest*>(ws);
    hipLaunchKernelGGL(hpe_upsample_kernel, dim3(bands, B), dim3(UP_TPB), 0, st, heat, h, w, cs, reinterpret_cast<float4*>(up),
                       part);
    if (int rc = mmh::check_launch("hpe_upsample")) return rc;
    hipLaunchKernelGGL(hpe_argmax_merge_kernel, dim3(B), dim3(64), 0, st, part, bands, w * UP, arg, maxv);
    return mmh::check_launch("hpe_argmax_merge");
}

int mmh_linear_chunks(int K) { return K >= 1 ? (int)mmh::cdiv(K, LIN_KC) : 0; }

size_t mmh_linear_fprop_ws_bytes(int M, int K, int N) {
    if (!lin_shape_ok(M, K, N)) return 0;
    return (size_t)mmh_linear_chunks(K) * M * N * sizeof(float);
}

int mmh_linear_fprop(const float* x, const float* wt, const float* bias, float* y, int M, int K, int N, int splits, void* ws,
                     size_t ws_bytes, mmh_stream_t s) {
    MMH_REQUIRE(x && wt && y && ws, "mmh_linear_fprop: NULL argument");
    MMH_REQUIRE(lin_shape_ok(M, K, N), "mmh_linear_fprop: bad shape M=%d K=%d N=%d (M <= 64, N %% 4 == 0)", M, K, N);
    const size_t need = mmh_linear_fprop_ws_bytes(M, K, N);
    MMH_REQUIRE(ws_bytes >= need, "mmh_linear_fprop: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(wt) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(ws) |
                  reinterpret_cast<uintptr_t>(bias)) & 15) == 0, "mmh_linear_fprop: w, bias, y and ws must be 16-byte aligned");
    const int chunks = mmh_linear_chunks(K);
    if (splits <= 0) splits = chunks;                    // one chunk per workgroup: the most parallel grid
    splits = std::min(splits, chunks);
    const int cps = (int)mmh::cdiv(chunks, splits);
    splits = (int)mmh::cdiv(chunks, cps);
    hipStream_t st = mmh::as_stream(s);
    float* slab = static_cast<float*>(ws);
    hipLaunchKernelGGL(hpe_linear_kernel, dim3((unsigned)mmh::cdiv(N, LIN_BN), splits), dim3(LIN_TPB), 0, st, x, wt, bias, M, K, N,
                       chunks, cps, slab);
    if (int rc = mmh::check_launch("hpe_linear")) return rc;
    const int64_t n4 = (int64_t)M * N / 4;
    return mmh::launch_slab_reduce(slab, y, n4, chunks, 0, n4, st);
}

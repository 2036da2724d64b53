// The two passes of the learned perceptual distance LPIPS (Zhang et al. 2018; the `lpips` package's LPIPS(net="vgg") in eval
// mode) that are not convolutions, for gfx950.  The VGG-16 trunk itself is mmh_conv2d_fprop + mmh_maxpool2x2_fwd
// (mmhand_amd/lpips.py).
//   * lpips_preprocess: an image in [-1, 1] (bytes: u / 255 * 2 - 1) through the package's ScalingLayer, (v - shift) / scale,
//     into the trunk's NHWC input.  float64, one rounding at the store.
//   * lpips_layer: the distance of two feature maps [B][H][W][C] at one tap.  Per pixel both vectors are normalised to unit
//     length and the squared difference is weighted by the tap's linear head; the layer's score is the mean over the pixels.
//     Both maps are read once.
//
// Layout of the layer kernel.  A pixel's C floats are C / 4 quads.  G = the smallest power of two >= min(C / 4, 64) lanes
// share a pixel; lane g of the group loads quad g (and quad g + 64 where C > 256) of a and of b with one 16-byte load each, so
// a wave reads 64 / G consecutive pixels = one contiguous run of both maps per instruction.  The two sums of squares and the
// weighted sum are butterflies over the group's lanes (xor G/2 .. 1) in float64: every lane of the group ends with the
// same bits, and a and b go through the same sequence, so swapping them changes nothing.  A workgroup of four waves visits
// 4 * 64 / G pixels at a time; workgroup k of an image takes visits k, k + chunks, ... and each lane adds its pixel's value to
// its own float64 accumulator in that order.  At the end: a butterfly over the wave's groups (xor 32 .. G), the four waves
// in order through LDS, one double per workgroup into the workspace.  A second launch adds an image's partials - thread t
// takes t, t + 256, ... in order, then a fixed tree - and divides by H W.  `chunks` follows from (H W, C) alone and the grid
// is (chunks, B): an image's result does not depend on the batch it is in.  No atomics.
#include <cmath>
#include "common.h"

namespace {

constexpr int LP_TPB = 256;              // four waves
constexpr int LP_MAX_CHUNKS = 1024;      // workgroups per image at most (the grid cap: beyond it a workgroup makes several visits)
constexpr int LP_FIN_TPB = 256;          // the finishing workgroup: partials per step
constexpr double LP_EPS = 1e-10;         // lpips.normalize_tensor's eps

__host__ __device__ inline int lp_group(int C) {
    const int q = C / 4;
    int g = 1;
    while (g < q && g < 64) g <<= 1;
    return g;
}

// pixels a workgroup visits at a time, and the workgroups of one image
inline int lp_visit_px(int C) { return (LP_TPB / 64) * (64 / lp_group(C)); }
inline int lp_chunks(int64_t px, int C) {
    const int64_t v = mmh::cdiv(px, lp_visit_px(C));
    return (int)(v < LP_MAX_CHUNKS ? v : LP_MAX_CHUNKS);
}

bool lp_shape_ok(int B, int H, int W, int C) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 4 && C <= 512 && C % 4 == 0 &&
           (int64_t)B * H * W * C < (int64_t(1) << 31);
}

// Loads are unconditional, from an address that is always valid (the caller clamps it), and a lane without a quad or a pixel
// turns what it loaded into zeros with a select where the value is USED: a branch around a load, or a select right behind
// it, makes the compiler wait for that load before it issues the next one
__device__ __forceinline__ float4 lp_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 lp_sel(const float4& v, bool ok) {
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

template <int G>
__device__ __forceinline__ double lp_group_sum(double v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double lp_sq4(const float4& v) {
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
    return ((x * x + y * y) + z * z) + w * w;
}

// sum over the quad's four channels of w (a / da - b / db)^2
__device__ __forceinline__ double lp_diff4(const float4& a, const float4& b, const float4& w, double da, double db) {
    const double t0 = (double)a.x / da - (double)b.x / db, t1 = (double)a.y / da - (double)b.y / db;
    const double t2 = (double)a.z / da - (double)b.z / db, t3 = (double)a.w / da - (double)b.w / db;
    return (((double)w.x * (t0 * t0) + (double)w.y * (t1 * t1)) + (double)w.z * (t2 * t2)) + (double)w.w * (t3 * t3);
}

// G lanes per pixel; TWO: a second quad per lane (C > 256, G == 64)
template <int G, bool TWO>
__global__ void __launch_bounds__(LP_TPB) lpips_layer_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                             const float* __restrict__ w, int px, int C, int chunks,
                                                             double* __restrict__ part) {
    __shared__ double sW[LP_TPB / 64];
    constexpr int PPW = 64 / G, VISIT = (LP_TPB / 64) * PPW;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane & (G - 1);
    const int b = blockIdx.y, chunk = blockIdx.x, quads = C >> 2;
    const bool q0 = g < quads, q1 = TWO && g + 64 < quads;
    // a lane without a quad, or without a pixel, loads quad 0 (of pixel 0 of its image) and selects zeros
    const int c0 = q0 ? 4 * g : 0, c1 = q1 ? 4 * (g + 64) : 0;
    const float4 w0 = lp_sel(lp_ld4(w + c0), q0), w1 = lp_sel(lp_ld4(w + c1), q1);
    const int64_t base = (int64_t)b * px * C;
    const int slot = wave * PPW + lane / G;          // this lane's pixel inside a visit
    const int visits = (px + VISIT - 1) / VISIT;
    float4 a0, b0, a1 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = a1;
    auto fetch = [&](int v) {                        // the loads of visit v, issued back to back
        const int p = v * VISIT + slot;
        const int64_t o = base + (int64_t)(p < px ? p : 0) * C;
        a0 = lp_ld4(fa + o + c0);
        b0 = lp_ld4(fb + o + c0);
        if (TWO) {
            a1 = lp_ld4(fa + o + c1);
            b1 = lp_ld4(fb + o + c1);
        }
    };
    double acc = 0.0;
    if (chunk < visits) fetch(chunk);
    for (int v = chunk; v < visits; v += chunks) {
        const bool in = v * VISIT + slot < px;       // a pixel past the end adds +0
        const float4 xa0 = lp_sel(a0, in && q0), xb0 = lp_sel(b0, in && q0), xa1 = lp_sel(a1, in && q1), xb1 = lp_sel(b1, in && q1);
        if (v + chunks < visits) fetch(v + chunks);  // the next visit's loads fly while this one is computed (v is uniform)
        double sa = lp_sq4(xa0), sb = lp_sq4(xb0);
        if (TWO) {
            sa = sa + lp_sq4(xa1);
            sb = sb + lp_sq4(xb1);
        }
        const double da = sqrt(lp_group_sum<G>(sa)) + LP_EPS, db = sqrt(lp_group_sum<G>(sb)) + LP_EPS;
        double d = lp_diff4(xa0, xb0, w0, da, db);
        if (TWO) d = d + lp_diff4(xa1, xb1, w1, da, db);
        acc = acc + lp_group_sum<G>(d);
    }
    // every lane of a group holds its pixel's sum: the wave's groups, then the waves
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) sW[wave] = acc;
    __syncthreads();
    if (tid == 0) part[(int64_t)b * chunks + chunk] = ((sW[0] + sW[1]) + sW[2]) + sW[3];
}

// workgroup = image: thread t adds partials t, t + 256, ... in order, then a fixed tree, one division
__global__ void __launch_bounds__(LP_FIN_TPB) lpips_finish_kernel(const double* __restrict__ part, int chunks, int px,
                                                                  double* __restrict__ out) {
    __shared__ double sP[LP_FIN_TPB];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int c = tid; c < chunks; c += LP_FIN_TPB) s = s + part[(int64_t)b * chunks + c];
    sP[tid] = s;
    __syncthreads();
    for (int n = LP_FIN_TPB / 2; n >= 1; n >>= 1) {
        if (tid < n) sP[tid] = sP[tid] + sP[tid + n];
        __syncthreads();
    }
    if (tid == 0) out[b] = sP[0] / (double)px;
}

template <int G, bool TWO>
void lp_launch(const float* fa, const float* fb, const float* w, int B, int px, int C, int chunks, double* part, hipStream_t st) {
    hipLaunchKernelGGL((lpips_layer_kernel<G, TWO>), dim3(chunks, B), dim3(LP_TPB), 0, st, fa, fb, w, px, C, chunks, part);
}

// ------------------------------------------------------------------------------------------------- preprocess
constexpr int PRE_TPB = 256;

template <typename T>
__device__ __forceinline__ double lp_px(const mmh_image_src& s, int64_t base, int c, int y, int x) {
    return (double)(float)reinterpret_cast<const T*>(s.ptr)[base + (int64_t)c * s.sc + (int64_t)y * s.sh + (int64_t)x * s.sw];
}

template <typename T, bool BYTES>
__global__ void __launch_bounds__(PRE_TPB) lpips_preprocess_kernel(mmh_image_src src, int H, int W, float4* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int64_t npx = (int64_t)H * W, p = (int64_t)blockIdx.x * PRE_TPB + threadIdx.x;
    if (p >= npx) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int64_t base = (int64_t)b * src.sb;
    // the ScalingLayer's constants: the float32 value of each literal, widened
    const double shift[3] = {(double)-.030f, (double)-.088f, (double)-.188f};
    const double scale[3] = {(double).458f, (double).448f, (double).450f};
    float z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v = lp_px<T>(src, base, c, y, x);
        if (BYTES) v = v / 255.0 * 2.0 - 1.0;
        z[c] = (float)((v - shift[c]) / scale[c]);
    }
    out[(int64_t)b * npx + p] = make_float4(z[0], z[1], z[2], 0.f);
}

template <typename T, bool BYTES>
int lp_launch_pre(const mmh_image_src& src, int B, int H, int W, float* out, hipStream_t st) {
    hipLaunchKernelGGL((lpips_preprocess_kernel<T, BYTES>), dim3((unsigned)mmh::cdiv((int64_t)H * W, PRE_TPB), B), dim3(PRE_TPB), 0,
                       st, src, H, W, reinterpret_cast<float4*>(out));
    return mmh::check_launch("lpips_preprocess");
}

}  // namespace

int mmh_lpips_preprocess(const mmh_image_src* src, int B, int H, int W, float* out, mmh_stream_t s) {
    MMH_REQUIRE(src && src->ptr && out, "mmh_lpips_preprocess: NULL argument");
    MMH_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t(1) << 31) &&
                    (int64_t)B * H * W * 4 < (int64_t(1) << 31),
                "mmh_lpips_preprocess: bad shape B=%d H=%d W=%d", B, H, W);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "mmh_lpips_preprocess: out must be 16-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    switch (src->dtype) {
        case MMH_F32: return lp_launch_pre<float, false>(*src, B, H, W, out, st);
        case MMH_BF16: return lp_launch_pre<__bf16, false>(*src, B, H, W, out, st);
        case MMH_FP16: return lp_launch_pre<_Float16, false>(*src, B, H, W, out, st);
        case MMH_U8: return lp_launch_pre<uint8_t, true>(*src, B, H, W, out, st);
        default: return mmh::fail("mmh_lpips_preprocess: unknown dtype %d", src->dtype);
    }
}

size_t mmh_lpips_layer_ws_bytes(int B, int H, int W, int C) {
    if (!lp_shape_ok(B, H, W, C)) return 0;
    return (size_t)B * lp_chunks((int64_t)H * W, C) * sizeof(double);
}

int mmh_lpips_layer(const float* fa, const float* fb, const float* w, int B, int H, int W, int C, double* out, void* ws,
                    size_t ws_bytes, mmh_stream_t s) {
    MMH_REQUIRE(fa && fb && w && out && ws, "mmh_lpips_layer: NULL argument");
    MMH_REQUIRE(lp_shape_ok(B, H, W, C), "mmh_lpips_layer: bad shape B=%d H=%d W=%d C=%d (C a multiple of 4 from 4 to 512, B <= 65535, "
                "fewer than 2^31 elements per map)", B, H, W, C);
    const size_t need = mmh_lpips_layer_ws_bytes(B, H, W, C);
    MMH_REQUIRE(ws_bytes >= need, "mmh_lpips_layer: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(fa) | reinterpret_cast<uintptr_t>(fb) | reinterpret_cast<uintptr_t>(w)) & 15) == 0 &&
                    ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "mmh_lpips_layer: fa, fb and w must be 16-byte aligned, out and the workspace 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    const int px = H * W, chunks = lp_chunks(px, C);
    double* part = static_cast<double*>(ws);
    switch (lp_group(C)) {
        case 1: lp_launch<1, false>(fa, fb, w, B, px, C, chunks, part, st); break;
        case 2: lp_launch<2, false>(fa, fb, w, B, px, C, chunks, part, st); break;
        case 4: lp_launch<4, false>(fa, fb, w, B, px, C, chunks, part, st); break;
        case 8: lp_launch<8, false>(fa, fb, w, B, px, C, chunks, part, st); break;
        case 16: lp_launch<16, false>(fa, fb, w, B, px, C, chunks, part, st); break;
        case 32: lp_launch<32, false>(fa, fb, w, B, px, C, chunks, part, st); break;
        default:
            if (C > 256) lp_launch<64, true>(fa, fb, w, B, px, C, chunks, part, st);
            else lp_launch<64, false>(fa, fb, w, B, px, C, chunks, part, st);
    }
    if (int rc = mmh::check_launch("lpips_layer")) return rc;
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(B), dim3(LP_FIN_TPB), 0, st, part, chunks, px, out);
    return mmh::check_launch("lpips_finish");
}

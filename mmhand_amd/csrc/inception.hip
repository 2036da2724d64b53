// The passes around Inception-v3's convolutions for the Inception score (baselines/quantitative_on_benchmarks/utils.py:22-28,
// 196-232 and inception.py), for gfx950.  All of them wait on memory or are tiny; none has an atomic, and every sum has an
// order that the grid does not enter.
//   * inception_preprocess: ToPILImage -> Resize(299) -> CenterCrop(299) -> ToTensor -> Normalize.  Two passes, as PIL's
//     ImagingResample runs them: a horizontal pass over the source rows into uint8, then a vertical pass over that.  Both are
//     integer: clip8(((1 << 21) + sum pixel * k) >> 22) with the host's 22-bit coefficients.  Only the columns and rows that the
//     centre-crop window reads are produced.  The last two transforms are a [3][256] table lookup.
//   * pool3x3: max (stride 2, no padding) and average (stride 1, zero padding 1, / 9) over NHWC lanes, into a concat buffer;
//     for pytorch-fid's graph (mmhand_amd/fid.py) also the average over the in-image pixels only and a stride-1 padded max.
//   * global_avgpool: the mean over an image's pixels, accumulated in float64 in pixel order.
//   * inception_score: float64 row softmax of the logits, the mean row py, and per row sum pyx * log(pyx / py).
#include <cmath>
#include "common.h"

namespace {

constexpr int TPB = 256;

// ------------------------------------------------------------------------------------------------- preprocess
constexpr int PIL_BITS = 22;     // ImagingResample's PRECISION_BITS for 8-bit images (32 - 8 - 2)

// a stored value -> the byte aug writes for it: ((v * 0.5 + 0.5) * 255).round().clamp(0, 255) in fp32, each operation rounded on
// its own, ties to even (torch.round)
template <typename T>
__device__ __forceinline__ int to_u8(T stored) {
#pragma clang fp contract(off)
    float t = (float)stored * 0.5f;
    t = t + 0.5f;
    t = t * 255.0f;
    t = rintf(t);
    return (int)fminf(fmaxf(t, 0.f), 255.f);     // a NaN becomes 0
}
template <>
__device__ __forceinline__ int to_u8<uint8_t>(uint8_t stored) { return stored; }

__device__ __forceinline__ int clip8(int v) {
    v >>= PIL_BITS;                               // arithmetic shift, as PIL's
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// horizontal pass: thread = (image, source row, window column); tmp [B][H][ow] of (r, g, b, 0) bytes.
// bounds[2 j] / bounds[2 j + 1]: first source column and tap count of resized column j; coefficients kk[j * ks + i].
template <typename T>
__global__ void __launch_bounds__(TPB) incep_resize_h_kernel(mmh_image_src src, int B, int H, int W, const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ kk, int ks, int crop_x, int ow,
                                                             uchar4* __restrict__ tmp) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= (int64_t)B * H * ow) return;
    const int ox = (int)(i % ow), y = (int)((i / ow) % H), b = (int)(i / ((int64_t)ow * H));
    const int j = crop_x + ox;
    const int x0 = bounds[2 * j], n = min(bounds[2 * j + 1], ks);
    const T* p = reinterpret_cast<const T*>(src.ptr) + (int64_t)b * src.sb + (int64_t)y * src.sh;
    int acc[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
    for (int t = 0; t < n; ++t) {
        const int x = min(max(x0 + t, 0), W - 1);          // the host's tables never leave the row; a bad table cannot either
        const int k = kk[(int64_t)j * ks + t];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += to_u8<T>(p[(int64_t)c * src.sc + (int64_t)x * src.sw]) * k;
    }
    tmp[i] = make_uchar4((unsigned char)clip8(acc[0]), (unsigned char)clip8(acc[1]), (unsigned char)clip8(acc[2]), 0);
}

// vertical pass + ToTensor + Normalize: thread = (image, window row, window column) -> out [B][oh][ow][4], lane 3 zero
__global__ void __launch_bounds__(TPB) incep_resize_v_kernel(const uchar4* __restrict__ tmp, int B, int H, const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ kk, int ks, int crop_y, int oh, int ow,
                                                             const float* __restrict__ lut, float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= (int64_t)B * oh * ow) return;
    const int ox = (int)(i % ow), oy = (int)((i / ow) % oh), b = (int)(i / ((int64_t)ow * oh));
    const int j = crop_y + oy;
    const int y0 = bounds[2 * j], n = min(bounds[2 * j + 1], ks);
    int acc[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
    for (int t = 0; t < n; ++t) {
        const int y = min(max(y0 + t, 0), H - 1);
        const int k = kk[(int64_t)j * ks + t];
        const uchar4 v = tmp[((int64_t)b * H + y) * ow + ox];
        acc[0] += (int)v.x * k;
        acc[1] += (int)v.y * k;
        acc[2] += (int)v.z * k;
    }
    out[i] = make_float4(lut[clip8(acc[0])], lut[256 + clip8(acc[1])], lut[512 + clip8(acc[2])], 0.f);
}

template <typename T>
int launch_preprocess(const mmh_image_src& src, int B, int H, int W, const int32_t* hb, const int32_t* hk, int hks,
                      const int32_t* vb, const int32_t* vk, int vks, int crop_y, int crop_x, int oh, int ow, const float* lut,
                      uchar4* tmp, float4* out, hipStream_t st) {
    hipLaunchKernelGGL(incep_resize_h_kernel<T>, dim3((unsigned)mmh::cdiv((int64_t)B * H * ow, TPB)), dim3(TPB), 0, st, src, B, H, W,
                       hb, hk, hks, crop_x, ow, tmp);
    if (int rc = mmh::check_launch("incep_resize_h")) return rc;
    hipLaunchKernelGGL(incep_resize_v_kernel, dim3((unsigned)mmh::cdiv((int64_t)B * oh * ow, TPB)), dim3(TPB), 0, st, tmp, B, H, vb,
                       vk, vks, crop_y, oh, ow, lut, out);
    return mmh::check_launch("incep_resize_v");
}

// ------------------------------------------------------------------------------------------------- pools
// thread = (image, output pixel, lane quad).  MAX: window rows 2 oy .. 2 oy + 2, all inside.  AVG: rows oy - 1 .. oy + 1, the
// ones inside summed in row-major order, the sum divided by 9 whatever their number (count_include_pad).  AVG_VALID: the same
// sum divided by the number of pixels inside (count_include_pad=False).  MAX_S1: the maximum over AVG's window.
template <int MODE>
__global__ void __launch_bounds__(TPB) pool3x3_kernel(const float* __restrict__ x, int B, int H, int W, int C4, int x_cs,
                                                      int Ho, int Wo, float* __restrict__ y, int y_cs) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= (int64_t)B * Ho * Wo * C4) return;
    const int q = (int)(i % C4);
    const int64_t px = i / C4;
    const int ox = (int)(px % Wo), oy = (int)((px / Wo) % Ho), b = (int)(px / ((int64_t)Wo * Ho));
    const int h0 = MODE == MMH_POOL_MAX ? 2 * oy : oy - 1, w0 = MODE == MMH_POOL_MAX ? 2 * ox : ox - 1;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    bool first = true;
    int inside = 0;
#pragma unroll
    for (int dh = 0; dh < 3; ++dh) {
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
            const int h = h0 + dh, w = w0 + dw;
            if (h < 0 || h >= H || w < 0 || w >= W) continue;
            const float4 v = *reinterpret_cast<const float4*>(x + (((int64_t)b * H + h) * W + w) * x_cs + q * 4);
            ++inside;
            if (first) {
                r = v;
                first = false;
            } else if (MODE == MMH_POOL_MAX || MODE == MMH_POOL_MAX_S1) {
                r.x = v.x > r.x ? v.x : r.x; r.y = v.y > r.y ? v.y : r.y; r.z = v.z > r.z ? v.z : r.z; r.w = v.w > r.w ? v.w : r.w;
            } else {
                r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
            }
        }
    }
    if (MODE == MMH_POOL_AVG) {
        // fp32 / fp32 through float64 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2), whatever the compiler's
        // fp32 division is
        r.x = (float)((double)r.x / 9.0); r.y = (float)((double)r.y / 9.0);
        r.z = (float)((double)r.z / 9.0); r.w = (float)((double)r.w / 9.0);
    }
    if (MODE == MMH_POOL_AVG_VALID) {       // 1 .. 9 pixels: the same correctly rounded quotient
        const double n = (double)inside;
        r.x = (float)((double)r.x / n); r.y = (float)((double)r.y / n);
        r.z = (float)((double)r.z / n); r.w = (float)((double)r.w / n);
    }
    *reinterpret_cast<float4*>(y + px * y_cs + q * 4) = r;
}

// thread = (image, channel): the image's pixels in order, float64
__global__ void __launch_bounds__(TPB) global_avgpool_kernel(const float* __restrict__ x, int B, int HW, int C, int x_cs,
                                                             float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= (int64_t)B * C) return;
    const int c = (int)(i % C), b = (int)(i / C);
    const float* p = x + (int64_t)b * HW * x_cs + c;
    double acc = 0.0;
    for (int k = 0; k < HW; ++k) acc += (double)p[(int64_t)k * x_cs];
    y[i] = (float)(acc / (double)HW);
}

// ------------------------------------------------------------------------------------------------- score
// the workgroup's 256 partial values, pairwise: a fixed tree.  Every thread returns the total.
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = TPB / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = MAX ? fmax(red[tid], red[tid + h]) : red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// workgroup = row: pyx[row][c] = exp(l[c] - max) / sum; thread t takes c = t, t + 256, ... in ascending order
__global__ void __launch_bounds__(TPB) score_softmax_kernel(const float* __restrict__ logits, int cs, int classes,
                                                            double* __restrict__ pyx) {
    __shared__ double red[TPB];
    const int64_t row = blockIdx.x;
    const float* l = logits + row * cs;
    double* o = pyx + row * classes;
    double mx = -INFINITY;
    for (int c = threadIdx.x; c < classes; c += TPB) mx = fmax(mx, (double)l[c]);
    mx = block_reduce<true>(mx, red);
    double sum = 0.0;
    for (int c = threadIdx.x; c < classes; c += TPB) {
        const double e = exp((double)l[c] - mx);
        o[c] = e;
        sum += e;
    }
    sum = block_reduce<false>(sum, red);
    for (int c = threadIdx.x; c < classes; c += TPB) o[c] = o[c] / sum;
}

// thread = class: the rows in row order
__global__ void __launch_bounds__(TPB) score_py_kernel(const double* __restrict__ pyx, int n, int classes, double* __restrict__ py) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= classes) return;
    double acc = 0.0;
    for (int64_t r = 0; r < n; ++r) acc += pyx[r * classes + c];
    py[c] = acc / (double)n;
}

// workgroup = row: kl[row] = sum pyx * log(pyx / py), terms with pyx == 0 are 0
__global__ void __launch_bounds__(TPB) score_kl_kernel(const double* __restrict__ pyx, const double* __restrict__ py, int classes,
                                                       double* __restrict__ kl) {
    __shared__ double red[TPB];
    const int64_t row = blockIdx.x;
    const double* p = pyx + row * classes;
    double sum = 0.0;
    for (int c = threadIdx.x; c < classes; c += TPB) {
        const double a = p[c];
        sum += a > 0.0 ? a * log(a / py[c]) : 0.0;
    }
    sum = block_reduce<false>(sum, red);
    if (threadIdx.x == 0) kl[row] = sum;
}

bool pre_shape_ok(int B, int H, int W, int oh, int ow) {
    return B >= 1 && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && (int64_t)B * H * ow < (int64_t(1) << 40) &&
           (int64_t)B * oh * ow < (int64_t(1) << 40) && mmh::cdiv((int64_t)B * H * ow, TPB) < (int64_t(1) << 31) &&
           mmh::cdiv((int64_t)B * oh * ow, TPB) < (int64_t(1) << 31);
}

}  // namespace

size_t mmh_inception_preprocess_ws_bytes(int B, int H, int W, int oh, int ow) {
    if (!pre_shape_ok(B, H, W, oh, ow)) return 0;
    return (size_t)B * H * ow * sizeof(uchar4);
}

int mmh_inception_preprocess(const mmh_image_src* src, int B, int H, int W, const int32_t* hbounds, const int32_t* hcoef, int hks,
                             int rw, const int32_t* vbounds, const int32_t* vcoef, int vks, int rh, int crop_y, int crop_x, int oh,
                             int ow, const float* lut, void* ws, size_t ws_bytes, float* out, mmh_stream_t s) {
    MMH_REQUIRE(src && src->ptr && hbounds && hcoef && vbounds && vcoef && lut && ws && out, "mmh_inception_preprocess: NULL argument");
    const size_t need = mmh_inception_preprocess_ws_bytes(B, H, W, oh, ow);
    MMH_REQUIRE(need > 0, "mmh_inception_preprocess: bad shape B=%d H=%d W=%d oh=%d ow=%d", B, H, W, oh, ow);
    MMH_REQUIRE(hks >= 1 && vks >= 1 && crop_y >= 0 && crop_x >= 0 && crop_y + oh <= rh && crop_x + ow <= rw,
                "mmh_inception_preprocess: window (%d,%d)+(%d,%d) outside the resized image %dx%d, or no taps", crop_y, crop_x, oh, ow,
                rh, rw);
    MMH_REQUIRE(ws_bytes >= need, "mmh_inception_preprocess: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                "mmh_inception_preprocess: out must be 16-byte and ws 4-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    uchar4* tmp = static_cast<uchar4*>(ws);
    float4* o = reinterpret_cast<float4*>(out);
#define MMH_PRE(T) launch_preprocess<T>(*src, B, H, W, hbounds, hcoef, hks, vbounds, vcoef, vks, crop_y, crop_x, oh, ow, lut, tmp, o, st)
    switch (src->dtype) {
        case MMH_F32: return MMH_PRE(float);
        case MMH_BF16: return MMH_PRE(__bf16);
        case MMH_FP16: return MMH_PRE(_Float16);
        case MMH_U8: return MMH_PRE(uint8_t);
        default: return mmh::fail("mmh_inception_preprocess: unknown dtype %d", src->dtype);
    }
#undef MMH_PRE
}

int mmh_pool3x3_fwd(const float* x, int B, int H, int W, int C, int x_cs, float* y, int y_cs, int mode, mmh_stream_t s) {
    MMH_REQUIRE(x && y, "mmh_pool3x3_fwd: NULL buffer");
    MMH_REQUIRE(mode == MMH_POOL_MAX || mode == MMH_POOL_AVG || mode == MMH_POOL_AVG_VALID || mode == MMH_POOL_MAX_S1,
                "mmh_pool3x3_fwd: mode %d (MMH_POOL_MAX | MMH_POOL_AVG | MMH_POOL_AVG_VALID | MMH_POOL_MAX_S1)", mode);
    MMH_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && x_cs % 4 == 0 && y_cs % 4 == 0 && x_cs >= C && y_cs >= C &&
                    (mode != MMH_POOL_MAX || (H >= 3 && W >= 3)),
                "mmh_pool3x3_fwd: bad shape B=%d H=%d W=%d C=%d x_cs=%d y_cs=%d (lanes in fours; max needs H, W >= 3)", B, H, W, C,
                x_cs, y_cs);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, "mmh_pool3x3_fwd: x and y must be 16-byte aligned");
    const int Ho = mode == MMH_POOL_MAX ? (H - 3) / 2 + 1 : H, Wo = mode == MMH_POOL_MAX ? (W - 3) / 2 + 1 : W;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    MMH_REQUIRE((int64_t)B * H * W * x_cs < (int64_t(1) << 40) && (int64_t)B * Ho * Wo * y_cs < (int64_t(1) << 40) &&
                    mmh::cdiv(total, TPB) < (int64_t(1) << 31), "mmh_pool3x3_fwd: tensor too large");
    const dim3 grid((unsigned)mmh::cdiv(total, TPB));
    if (mode == MMH_POOL_MAX)
        hipLaunchKernelGGL(pool3x3_kernel<MMH_POOL_MAX>, grid, dim3(TPB), 0, mmh::as_stream(s), x, B, H, W, C / 4, x_cs, Ho, Wo, y, y_cs);
    else if (mode == MMH_POOL_AVG_VALID)
        hipLaunchKernelGGL(pool3x3_kernel<MMH_POOL_AVG_VALID>, grid, dim3(TPB), 0, mmh::as_stream(s), x, B, H, W, C / 4, x_cs, Ho, Wo, y, y_cs);
    else if (mode == MMH_POOL_MAX_S1)
        hipLaunchKernelGGL(pool3x3_kernel<MMH_POOL_MAX_S1>, grid, dim3(TPB), 0, mmh::as_stream(s), x, B, H, W, C / 4, x_cs, Ho, Wo, y, y_cs);
    else
        hipLaunchKernelGGL(pool3x3_kernel<MMH_POOL_AVG>, grid, dim3(TPB), 0, mmh::as_stream(s), x, B, H, W, C / 4, x_cs, Ho, Wo, y, y_cs);
    return mmh::check_launch("pool3x3");
}

int mmh_global_avgpool(const float* x, int B, int H, int W, int C, int x_cs, float* y, mmh_stream_t s) {
    MMH_REQUIRE(x && y, "mmh_global_avgpool: NULL buffer");
    MMH_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && x_cs >= C && (int64_t)H * W < (int64_t(1) << 31) &&
                    (int64_t)B * H * W * x_cs < (int64_t(1) << 40) && mmh::cdiv((int64_t)B * C, TPB) < (int64_t(1) << 31),
                "mmh_global_avgpool: bad shape B=%d H=%d W=%d C=%d x_cs=%d", B, H, W, C, x_cs);
    hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)mmh::cdiv((int64_t)B * C, TPB)), dim3(TPB), 0, mmh::as_stream(s), x, B,
                       H * W, C, x_cs, y);
    return mmh::check_launch("global_avgpool");
}

size_t mmh_inception_score_ws_bytes(int n, int classes) {
    if (n < 1 || classes < 1 || (int64_t)n * classes >= (int64_t(1) << 40)) return 0;
    return (size_t)n * classes * sizeof(double);
}

int mmh_inception_score(const float* logits, int n, int cs, int classes, double* kl, double* py, void* ws, size_t ws_bytes,
                        mmh_stream_t s) {
    MMH_REQUIRE(logits && kl && py && ws, "mmh_inception_score: NULL argument");
    const size_t need = mmh_inception_score_ws_bytes(n, classes);
    MMH_REQUIRE(need > 0 && cs >= classes, "mmh_inception_score: bad shape n=%d cs=%d classes=%d", n, cs, classes);
    MMH_REQUIRE(ws_bytes >= need, "mmh_inception_score: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(kl) | reinterpret_cast<uintptr_t>(py)) & 7) == 0,
                "mmh_inception_score: kl, py and ws must be 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    double* pyx = static_cast<double*>(ws);
    hipLaunchKernelGGL(score_softmax_kernel, dim3(n), dim3(TPB), 0, st, logits, cs, classes, pyx);
    if (int rc = mmh::check_launch("score_softmax")) return rc;
    hipLaunchKernelGGL(score_py_kernel, dim3((unsigned)mmh::cdiv(classes, TPB)), dim3(TPB), 0, st, pyx, n, classes, py);
    if (int rc = mmh::check_launch("score_py")) return rc;
    hipLaunchKernelGGL(score_kl_kernel, dim3(n), dim3(TPB), 0, st, pyx, py, classes, kl);
    return mmh::check_launch("score_kl");
}

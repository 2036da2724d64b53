// Conventional augmentation of the hand-pose estimators' training input (train_hpe --augment_geom / --augment_color), for
// gfx950: mmh_hpe_augment_normalize turns a uint8 BGR batch into the estimators' NHWC input under a per-image inverse affine
// map, a per-image 3x3 colour matrix and a per-image gamma, and takes cv2.normalize(NORM_MINMAX)'s minimum and maximum
// AFTER them, over the warped output.  [The min-max normalisation cancels every change of brightness or contrast that is one
// affine map of all three channels, so the colour operations mix channels or are non-linear, and they cannot be a pre-pass in
// front of mmh_hpe_normalize's own reduction over the source.]
//
// Two passes, both recomputing the value of a pixel from the source bytes (aug_value, the one definition):
//   1. hpe_aug_minmax_kernel: chunk c of image b visits the output pixels c * 256 + tid, + chunks * 256, ... and leaves
//      (min, max) of its values in ws; at most AUG_MAX_CHUNKS chunks per image.
//   2. hpe_aug_write_kernel: every workgroup of image b folds the image's partials in order and writes its 256 pixels.
// Per output pixel that is 2 x (up to 12 source bytes, neighbours sharing them in cache) read and 16 bytes written; keeping
// the three float64 values in ws between the passes would write 24, read 24 and write 16.  Minimum and maximum
// are exact in any order; there is still no atomic.
#include <cmath>
#include "affine_sample.h"

namespace {
using namespace mmh::dev;

constexpr int AUG_TPB = 256;
constexpr int AUG_MAX_CHUNKS = 64;

__host__ __device__ inline int aug_chunks(int Ho, int Wo) {
    const int64_t px = (int64_t)Ho * Wo;
    const int64_t c = (px + AUG_TPB - 1) / AUG_TPB;
    return (int)(c < AUG_MAX_CHUNKS ? c : AUG_MAX_CHUNKS);
}

// one row of the colour matrix on (R, G, B): each product and sum rounded on its own, as affine_coord does it
__device__ __forceinline__ double color_row(const double* __restrict__ m, double R, double G, double B) {
#pragma clang fp contract(off)
    return (m[0] * R + m[1] * G) + m[2] * B;
}

struct AugArgs {
    const uint8_t* img;
    const double* xf;       // [B][6] or NULL
    const double* cm;       // [B][9] or NULL
    const double* gamma;    // [B] or NULL
    int Hs, Ws, Ho, Wo, chunks;
};

// the maps of image b in registers: a = its sampling matrix (xf == NULL: the identity), m = its colour matrix when there is one
struct AugMaps { const uint8_t* img; double a[6], m[9], g; bool has_cm; };
__device__ __forceinline__ AugMaps aug_maps(const AugArgs& p, int b) {
    AugMaps k;
    k.img = p.img + (int64_t)b * p.Hs * p.Ws * 3;
#pragma unroll
    for (int i = 0; i < 6; ++i) k.a[i] = p.xf ? p.xf[(int64_t)b * 6 + i] : (i == 0 || i == 4 ? 1.0 : 0.0);
    k.has_cm = p.cm != nullptr;
#pragma unroll
    for (int i = 0; i < 9; ++i) k.m[i] = k.has_cm ? p.cm[(int64_t)b * 9 + i] : 0.0;
    k.g = p.gamma ? p.gamma[b] : 1.0;
    return k;
}

// The value of output pixel (x, y) of one image before the normalisation, v[0..2] = R, G, B in [0, 255]: sampled through k.a,
// through the colour matrix k.m (none = identity), clamped, through the gamma curve (g == 1: no pow).
__device__ __forceinline__ void aug_value(const AugMaps& k, int x, int y, int Hs, int Ws, double v[3]) {
    const uint8_t* __restrict__ img = k.img;
    const AffineTaps t = affine_taps(k.a, x, y, Hs, Ws);
    double c[3];                                                    // R, G, B out of B, G, R bytes
#pragma unroll
    for (int e = 0; e < 3; ++e)
        c[e] = lerp2((double)img[t.o00 + 2 - e], (double)img[t.o01 + 2 - e], (double)img[t.o10 + 2 - e],
                     (double)img[t.o11 + 2 - e], t.wx, t.wy);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        double r = k.has_cm ? color_row(k.m + 3 * e, c[0], c[1], c[2]) : c[e];
        r = r > 0.0 ? r : 0.0;                                      // NaN compares false: 0
        r = r < 255.0 ? r : 255.0;
        if (k.g != 1.0) r = 255.0 * pow(r / 255.0, k.g);
        v[e] = r;
    }
}

__global__ void __launch_bounds__(AUG_TPB) hpe_aug_minmax_kernel(AugArgs p, double* __restrict__ part) {
    __shared__ double red_mn[AUG_TPB], red_mx[AUG_TPB];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const AugMaps k = aug_maps(p, b);
    const int64_t npx = (int64_t)p.Ho * p.Wo;
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t q = (int64_t)chunk * AUG_TPB + tid; q < npx; q += (int64_t)p.chunks * AUG_TPB) {
        const int y = (int)(q / p.Wo), x = (int)(q - (int64_t)y * p.Wo);
        double v[3];
        aug_value(k, x, y, p.Hs, p.Ws, v);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            mn = fmin(mn, v[e]);
            mx = fmax(mx, v[e]);
        }
    }
    red_mn[tid] = mn;
    red_mx[tid] = mx;
    __syncthreads();
    for (int h = AUG_TPB / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red_mn[tid] = fmin(red_mn[tid], red_mn[tid + h]);
            red_mx[tid] = fmax(red_mx[tid], red_mx[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t i = ((int64_t)b * p.chunks + chunk) * 2;
        part[i] = red_mn[0];
        part[i + 1] = red_mx[0];
    }
}

__global__ void __launch_bounds__(AUG_TPB) hpe_aug_write_kernel(AugArgs p, const double* __restrict__ part,
                                                                float4* __restrict__ out) {
    const int b = blockIdx.y;
    double mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < p.chunks; ++i) {
        const int64_t j = ((int64_t)b * p.chunks + i) * 2;
        mn = fmin(mn, part[j]);
        mx = fmax(mx, part[j + 1]);
    }
    const int64_t npx = (int64_t)p.Ho * p.Wo;
    const int64_t q = (int64_t)blockIdx.x * AUG_TPB + threadIdx.x;
    if (q >= npx) return;
    const AugMaps k = aug_maps(p, b);
    const int y = (int)(q / p.Wo), x = (int)(q - (int64_t)y * p.Wo);
    double v[3];
    aug_value(k, x, y, p.Hs, p.Ws, v);
    const double range = mx - mn;
    float o[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = range > 0.0 ? (float)((v[e] - mn) / range) : 0.f;
    out[(int64_t)b * npx + q] = make_float4(o[0], o[1], o[2], 0.f);
}

}  // namespace

size_t mmh_hpe_augment_normalize_ws_bytes(int B, int Ho, int Wo) {
    if (B < 1 || B > 65535 || Ho < 1 || Wo < 1 || (int64_t)Ho * Wo >= (int64_t(1) << 31)) return 0;
    return (size_t)B * aug_chunks(Ho, Wo) * 2 * sizeof(double);
}

int mmh_hpe_augment_normalize(const void* img, int B, int Hs, int Ws, int Ho, int Wo, const double* xf, const double* cm,
                              const double* gamma, void* ws, size_t ws_bytes, float* out, mmh_stream_t s) {
    MMH_REQUIRE(img && ws && out, "mmh_hpe_augment_normalize: NULL buffer");
    const size_t need = mmh_hpe_augment_normalize_ws_bytes(B, Ho, Wo);
    MMH_REQUIRE(need > 0 && Hs > 0 && Ws > 0 && (int64_t)Hs * Ws < (int64_t(1) << 31),
                "mmh_hpe_augment_normalize: bad shape B=%d Hs=%d Ws=%d Ho=%d Wo=%d", B, Hs, Ws, Ho, Wo);
    MMH_REQUIRE(xf || (Ho == Hs && Wo == Ws), "mmh_hpe_augment_normalize: xf = NULL needs an output of the source's size");
    MMH_REQUIRE(ws_bytes >= need, "mmh_hpe_augment_normalize: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "mmh_hpe_augment_normalize: out must be 16-byte aligned");
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(xf) | reinterpret_cast<uintptr_t>(cm) | reinterpret_cast<uintptr_t>(gamma) |
                  reinterpret_cast<uintptr_t>(ws)) & 7) == 0, "mmh_hpe_augment_normalize: xf, cm, gamma and ws must be 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    AugArgs p;
    p.img = static_cast<const uint8_t*>(img), p.xf = xf, p.cm = cm, p.gamma = gamma;
    p.Hs = Hs, p.Ws = Ws, p.Ho = Ho, p.Wo = Wo, p.chunks = aug_chunks(Ho, Wo);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(hpe_aug_minmax_kernel, dim3(p.chunks, B), dim3(AUG_TPB), 0, st, p, part);
    if (int rc = mmh::check_launch("hpe_aug_minmax")) return rc;
    hipLaunchKernelGGL(hpe_aug_write_kernel, dim3((unsigned)mmh::cdiv((int64_t)Ho * Wo, AUG_TPB), B), dim3(AUG_TPB), 0, st, p, part,
                       reinterpret_cast<float4*>(out));
    return mmh::check_launch("hpe_aug_write");
}

// Image quality metrics for gfx950: per-image SSIM (pytorch_ssim/__init__.py:17-37, size_average=False as the Evaluator
// calls it per image, utils.py:100-111), mean |a-b| and mean (a-b)^2 of image pairs mapped to [0, 1].
//
// One workgroup per (output tile 32x32, channel, image): both images' (32+w-1)^2 halo goes to LDS once (zero padding and
// the [0, 1] mapping on the way in), a horizontal pass writes the five moment rows (a, b, a^2, b^2, ab) of the 32 output
// columns for every halo row, a vertical pass finishes the 2-D Gaussian, and the SSIM map, |a-b| and (a-b)^2 are reduced
// per workgroup in float64.  A second kernel reduces an image's partials in a fixed order in float64.  No atomics: the
// result of an image depends on its own pixels only and is bit-identical from run to run.
//
// Accuracy: sigma^2 = E[x^2] - mu^2 cancels against C2 = 9e-4 on flat regions.  fp32 moments are accurate only of values
// centred near the pixel they describe: one shift per tile is not enough (a saturated +1 block on a -1 background missed
// float64 by 2e-6 with one shift per 32x32 tile).  So every moment is taken about a pixel inside its own window:
//  * horizontal pass: the row moments of output columns 2j, 2j+1 are of values shifted by the halo pixel of column 2j in
//    that row (K_r, inside both row windows);
//  * vertical pass: each row's moments are moved to the centre c of a group of output pixels of one column (the pixel of
//    the group's second row; every output of the group is within w/2 rows of it) with the exact identities
//      sum g (x - c)   = h1 + d s,   sum g (x - c)^2 = h2 + 2 d (h1 + d s/2),
//      sum g (xa - ca)(xb - cb) = hab + da (h1b + db s/2) + db (h1a + da s/2),     d = K_r - c, s = sum of the taps,
//    before the vertical taps add them up.
// On a flat region every term is then of the size of the noise, and where the terms are large (an edge inside the window)
// so is the variance.  In exact arithmetic the sigma terms do not depend on the shift when the window sums to 1.  The
// window does not sum to 1 exactly (its taps are fp32, as the reference builds them; the caller passes them, because their
// last bit is decided by torch's fp32 summation order, and S - 1 moves a flat region's SSIM by up to (S - 1) / C2): the
// leftover, (S - 1) c (2 mu' + S c), is taken out again with S - 1 computed on the host in float64, so the kernel follows
// the reference's formula evaluated in exact arithmetic.
//
// Symmetry: the a and b paths are the same instructions, and the cross terms and the combination are written without
// contraction in mirror-image form, so ssim(a, b) == ssim(b, a) bit for bit and ssim(x, x) == 1 exactly.
#include <cmath>
#include "common.h"

namespace {

constexpr int MT = 32;           // output tile edge
constexpr int MTPB = 256;        // threads per workgroup: 32 columns x 8 groups of 4 rows
constexpr int MROW = 48;         // LDS row stride of the halo (>= 32 + 15 - 1)
constexpr int HROW = 34;         // LDS row stride of the horizontal moments (8-byte rows, no bank conflict 4 rows apart)

struct MetricTaps {
    float g[16];                 // 1-D taps, normalised in fp32 as pytorch_ssim.gaussian
    float s, s2;                 // their sum (fp32) and half of it
    float sm1;                   // (sum of the 2-D window) - 1, from float64 on the host
    float c1, c2;
};

// both images' (R x R) halos of their channel planes -> LDS (row stride MROW), mapped to [0, 1], zero outside the image.
// The dtypes are resolved once per call, and every load of a thread is issued before the first one is waited for.
template <typename TA, typename TB, int R>
__device__ __forceinline__ void load_halos_t(const mmh_image_src& A, int64_t baseA, const mmh_image_src& B, int64_t baseB,
                                             int y0, int x0, int H, int W, float2* dAB) {
    constexpr int N = (R * R + MTPB - 1) / MTPB;
    const TA* pa = reinterpret_cast<const TA*>(A.ptr) + baseA;
    const TB* pb = reinterpret_cast<const TB*>(B.ptr) + baseB;
    float va[N], vb[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int i = threadIdx.x + k * MTPB;
        const int r = i / R, q = i - r * R;
        const int y = y0 + r, x = x0 + q;
        va[k] = vb[k] = 0.f;
        if (i < R * R && y >= 0 && y < H && x >= 0 && x < W) {
            va[k] = __builtin_fmaf((float)pa[(int64_t)y * A.sh + (int64_t)x * A.sw], A.scale, A.offset);
            vb[k] = __builtin_fmaf((float)pb[(int64_t)y * B.sh + (int64_t)x * B.sw], B.scale, B.offset);
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int i = threadIdx.x + k * MTPB;
        const int r = i / R, q = i - r * R;
        if (i < R * R) {
            dAB[r * MROW + q] = make_float2(va[k], vb[k]);
        }
    }
}

template <typename TA, int R>
__device__ __forceinline__ void load_halos_b(const mmh_image_src& A, int64_t baseA, const mmh_image_src& B, int64_t baseB,
                                             int y0, int x0, int H, int W, float2* dAB) {
    switch (B.dtype) {
        case MMH_BF16: load_halos_t<TA, __bf16, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
        case MMH_FP16: load_halos_t<TA, _Float16, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
        case MMH_U8: load_halos_t<TA, uint8_t, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
        default: load_halos_t<TA, float, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
    }
}

template <int R>
__device__ __forceinline__ void load_halos(const mmh_image_src& A, int64_t baseA, const mmh_image_src& B, int64_t baseB,
                                           int y0, int x0, int H, int W, float2* dAB) {
    switch (A.dtype) {
        case MMH_BF16: load_halos_b<__bf16, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
        case MMH_FP16: load_halos_b<_Float16, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
        case MMH_U8: load_halos_b<uint8_t, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
        default: load_halos_b<float, R>(A, baseA, B, baseB, y0, x0, H, W, dAB); break;
    }
}

// SSIM of one pixel from its moments about (ca, cb) (m = a', b', a'^2, b'^2, a'b').  No contraction: every expression is
// evaluated as written, the a and b operands in mirror-image positions.
__device__ __forceinline__ float ssim_px(const float* m, float ca, float cb, const MetricTaps& t) {
#pragma clang fp contract(off)
    const float ma = m[0], mb = m[1], e = t.sm1;
    const float ua = (ma + ca) + ca * e;                         // mu = mu' + S c
    const float ub = (mb + cb) + cb * e;
    const float caa = e * ((ca * ma + ca * ma) + ca * ca);       // (S - 1)(2 c mu' + c^2)
    const float cbb = e * ((cb * mb + cb * mb) + cb * cb);
    const float cab = e * ((ca * mb + cb * ma) + ca * cb);
    const float saa = (m[2] - ma * ma) - caa;
    const float sbb = (m[3] - mb * mb) - cbb;
    const float sab = (m[4] - ma * mb) - cab;
    const float num = (2.f * (ua * ub) + t.c1) * (2.f * sab + t.c2);
    const float den = ((ua * ua + ub * ub) + t.c1) * ((saa + sbb) + t.c2);
    return num / den;
}

// one halo row's moments (h = a', b', a'^2, b'^2, a'b' about the row shifts) moved to the group centre: d = K_r - c
__device__ __forceinline__ void recentre(const float* h, float da, float db, const MetricTaps& t, float* m) {
#pragma clang fp contract(off)
    const float pa = __builtin_fmaf(da, t.s2, h[0]), pb = __builtin_fmaf(db, t.s2, h[1]);
    m[0] = __builtin_fmaf(da, t.s, h[0]);
    m[1] = __builtin_fmaf(db, t.s, h[1]);
    const float xa = da * pa, xb = db * pb;
    m[2] = (xa + xa) + h[2];
    m[3] = (xb + xb) + h[3];
    m[4] = (da * pb + db * pa) + h[4];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int WIN>
__global__ void __launch_bounds__(MTPB) image_metrics_tile_kernel(mmh_image_src A, mmh_image_src Bsrc, int C, int H, int W,
                                                                  int tiles_x, MetricTaps taps, double* __restrict__ part) {
    constexpr int R = MT + WIN - 1;   // halo rows / columns
    constexpr int HALF = WIN / 2;
    constexpr int GV = WIN >= 5 ? 4 : 2;   // output rows per vertical group: every one within HALF rows of the centre
    __shared__ float2 sAB[R * MROW];      // the two halos interleaved: one 8-byte LDS read per pixel pair
    __shared__ __attribute__((aligned(16))) float sH[5 * R * HROW];
    __shared__ double sRed[MTPB / 64][3];

    const int tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int y0 = (tile / tiles_x) * MT, x0 = (tile % tiles_x) * MT;
    const int tid = threadIdx.x;
    const int64_t baseA = (int64_t)b * A.sb + (int64_t)c * A.sc;
    const int64_t baseB = (int64_t)b * Bsrc.sb + (int64_t)c * Bsrc.sc;

    // halo -> LDS, mapped to [0, 1]; zero outside the image
    load_halos<R>(A, baseA, Bsrc, baseB, y0 - HALF, x0 - HALF, H, W, sAB);
    __syncthreads();

    // horizontal pass: row r, output columns 2 xg, 2 xg + 1, five moments of the values shifted by the halo pixel at the
    // centre of column 2 xg's row window (R * 16 items: 2.6 rounds of 256 threads at w = 11)
    for (int it = tid; it < R * (MT / 2); it += MTPB) {
        const int r = it >> 4, xg = it & 15;
        const float2* rab = sAB + r * MROW + xg * 2;
        const float ka = rab[HALF].x, kb = rab[HALF].y;
        float va[WIN + 1], vb[WIN + 1];
#pragma unroll
        for (int j = 0; j < WIN + 1; ++j) {
            const float2 v = rab[j];
            va[j] = v.x - ka;
            vb[j] = v.y - kb;
        }
        float acc[5][2];
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[m][0] = acc[m][1] = 0.f;
#pragma unroll
        for (int j = 0; j < WIN + 1; ++j) {
            const float aa = va[j] * va[j], bb = vb[j] * vb[j], ab = va[j] * vb[j];
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int k = j - o;
                if (k >= 0 && k < WIN) {
                    const float g = taps.g[k];
                    acc[0][o] = __builtin_fmaf(g, va[j], acc[0][o]);
                    acc[1][o] = __builtin_fmaf(g, vb[j], acc[1][o]);
                    acc[2][o] = __builtin_fmaf(g, aa, acc[2][o]);
                    acc[3][o] = __builtin_fmaf(g, bb, acc[3][o]);
                    acc[4][o] = __builtin_fmaf(g, ab, acc[4][o]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
            *reinterpret_cast<float2*>(sH + (m * R + r) * HROW + xg * 2) = make_float2(acc[m][0], acc[m][1]);
    }
    __syncthreads();

    // vertical pass: column tx, output rows 4 ty .. 4 ty + 3 in groups of GV rows about the pixel of the group's second row
    const int tx = tid & 31, ty = tid >> 5;
    const int kcol = (tx & ~1) + HALF;              // halo column of this column's horizontal shifts
    float mom[4][5], cenA[4], cenB[4];
#pragma unroll
    for (int g0 = 0; g0 < 4; g0 += GV) {
        const int row0 = ty * 4 + g0;                // halo row of the group's first window row
        const float2 cc = sAB[(row0 + 1 + HALF) * MROW + tx + HALF];
        const float ca = cc.x, cb = cc.y;
        float acc[GV][5];
#pragma unroll
        for (int o = 0; o < GV; ++o)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[o][m] = 0.f;
#pragma unroll
        for (int j = 0; j < WIN + GV - 1; ++j) {
            const int r = row0 + j;
            float h[5], mr[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) h[m] = sH[(m * R + r) * HROW + tx];
            const float2 kr = sAB[r * MROW + kcol];
            recentre(h, kr.x - ca, kr.y - cb, taps, mr);
#pragma unroll
            for (int o = 0; o < GV; ++o) {
                const int k = j - o;
                if (k >= 0 && k < WIN)
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[o][m] = __builtin_fmaf(taps.g[k], mr[m], acc[o][m]);
            }
        }
#pragma unroll
        for (int o = 0; o < GV; ++o) {
#pragma unroll
            for (int m = 0; m < 5; ++m) mom[g0 + o][m] = acc[o][m];
            cenA[g0 + o] = ca;
            cenB[g0 + o] = cb;
        }
    }
    double s_ssim = 0.0, s_l1 = 0.0, s_se = 0.0;
    const int ox = x0 + tx;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int oy = y0 + ty * 4 + o;
        if (oy < H && ox < W) {
            s_ssim += (double)ssim_px(mom[o], cenA[o], cenB[o], taps);
            const int li = (ty * 4 + o + HALF) * MROW + tx + HALF;
            const double d = (double)sAB[li].x - (double)sAB[li].y;
            s_l1 += fabs(d);
            s_se += d * d;
        }
    }
    s_ssim = wave_sum(s_ssim);
    s_l1 = wave_sum(s_l1);
    s_se = wave_sum(s_se);
    const int wv = tid >> 6;
    if ((tid & 63) == 0) {
        sRed[wv][0] = s_ssim;
        sRed[wv][1] = s_l1;
        sRed[wv][2] = s_se;
    }
    __syncthreads();
    if (tid == 0) {
        double* p = part + (((int64_t)b * C + c) * (int64_t)gridDim.x + tile) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double t = sRed[0][k];
#pragma unroll
            for (int w = 1; w < MTPB / 64; ++w) t += sRed[w][k];
            p[k] = t;
        }
    }
}

// one workgroup per image: its n partials in a fixed order (strided per thread, then a fixed tree), divided by C H W
__global__ void __launch_bounds__(256) image_metrics_final_kernel(const double* __restrict__ part, int n, double inv_count,
                                                                  double* __restrict__ out) {
    __shared__ double sRed[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* p = part + (int64_t)b * n * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += p[(int64_t)i * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) sRed[k][tid] = s[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
#pragma unroll
            for (int k = 0; k < 3; ++k) sRed[k][tid] += sRed[k][tid + h];
        __syncthreads();
    }
    if (tid < 3) out[(int64_t)b * 3 + tid] = sRed[tid][0] * inv_count;
}

int64_t metric_tiles(int H, int W) { return mmh::cdiv(H, MT) * mmh::cdiv(W, MT); }

bool metric_shape_ok(int B, int C, int H, int W, int window) {
    return B >= 1 && B <= 65535 && C >= 1 && C <= 65535 && H >= 1 && W >= 1 && window >= 3 && window <= 15 &&
           window % 2 == 1 &&
           // the launch: tiles * 256 work-items in grid dimension x (< 2^32); the final kernel's int count of partials
           metric_tiles(H, W) * MTPB < (int64_t(1) << 32) && (int64_t)C * metric_tiles(H, W) < (int64_t(1) << 31);
}

template <int WIN>
void launch_tiles(const mmh_image_src& a, const mmh_image_src& b, int B, int C, int H, int W, const MetricTaps& t,
                  double* part, hipStream_t s) {
    const int tiles_x = (int)mmh::cdiv(W, MT);
    hipLaunchKernelGGL(image_metrics_tile_kernel<WIN>, dim3((unsigned)metric_tiles(H, W), C, B), dim3(MTPB), 0, s, a, b, C, H, W,
                       tiles_x, t, part);
}

}  // namespace

size_t mmh_image_metrics_ws_bytes(int B, int C, int H, int W, int window) {
    if (!metric_shape_ok(B, C, H, W, window)) return 0;
    return (size_t)B * C * metric_tiles(H, W) * 3 * sizeof(double);
}

int mmh_image_metrics(const mmh_image_src* a, const mmh_image_src* b, int B, int C, int H, int W, int window, const float* taps,
                      double c1, double c2, void* ws, size_t ws_bytes, double* out, mmh_stream_t s) {
    MMH_REQUIRE(a && b && a->ptr && b->ptr && ws && out, "mmh_image_metrics: NULL argument");
    MMH_REQUIRE(window >= 3 && window <= 15 && window % 2 == 1, "mmh_image_metrics: window %d (odd, 3 .. 15)", window);
    MMH_REQUIRE(metric_shape_ok(B, C, H, W, window), "mmh_image_metrics: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    MMH_REQUIRE(taps && c1 > 0 && c2 > 0, "mmh_image_metrics: taps must be given, c1 and c2 > 0");
    double tsum = 0.0;
    for (int i = 0; i < window; ++i) {
        MMH_REQUIRE(taps[i] > 0.f && taps[i] < 1.f, "mmh_image_metrics: tap %d = %g (a normalised window has taps in (0, 1))", i,
                    (double)taps[i]);
        tsum += taps[i];
    }
    MMH_REQUIRE(std::fabs(tsum - 1.0) < 1e-5, "mmh_image_metrics: the taps sum to %.9g, not 1", tsum);
    for (const mmh_image_src* p : {a, b})
        MMH_REQUIRE(p->dtype == MMH_F32 || p->dtype == MMH_BF16 || p->dtype == MMH_FP16 || p->dtype == MMH_U8,
                    "mmh_image_metrics: unknown dtype %d", p->dtype);
    const size_t need = mmh_image_metrics_ws_bytes(B, C, H, W, window);
    MMH_REQUIRE(need > 0 && ws_bytes >= need, "mmh_image_metrics: workspace %zu bytes < %zu", ws_bytes, need);

    // the 2-D window is the fp32 outer product of the taps (pytorch_ssim.create_window); its sum, in float64, gives S - 1
    MetricTaps t{};
    float tsum32 = 0.f;
    for (int i = 0; i < window; ++i) {
        t.g[i] = taps[i];
        tsum32 += taps[i];
    }
    t.s = tsum32;
    t.s2 = 0.5f * tsum32;
    double s2 = 0.0;
    for (int i = 0; i < window; ++i)
        for (int j = 0; j < window; ++j) s2 += (double)(t.g[i] * t.g[j]);
    t.sm1 = (float)(s2 - 1.0);
    t.c1 = (float)c1;
    t.c2 = (float)c2;

    hipStream_t st = mmh::as_stream(s);
    double* part = static_cast<double*>(ws);
    switch (window) {
        case 3: launch_tiles<3>(*a, *b, B, C, H, W, t, part, st); break;
        case 5: launch_tiles<5>(*a, *b, B, C, H, W, t, part, st); break;
        case 7: launch_tiles<7>(*a, *b, B, C, H, W, t, part, st); break;
        case 9: launch_tiles<9>(*a, *b, B, C, H, W, t, part, st); break;
        case 11: launch_tiles<11>(*a, *b, B, C, H, W, t, part, st); break;
        case 13: launch_tiles<13>(*a, *b, B, C, H, W, t, part, st); break;
        default: launch_tiles<15>(*a, *b, B, C, H, W, t, part, st); break;
    }
    if (int rc = mmh::check_launch("image_metrics_tile")) return rc;
    const int n = (int)(C * metric_tiles(H, W));
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3(B), dim3(256), 0, st, part, n, 1.0 / ((double)C * H * W), out);
    return mmh::check_launch("image_metrics_final");
}

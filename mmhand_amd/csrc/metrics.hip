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
#include <algorithm>
#include <cmath>
#include <type_traits>
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

// The four factors of one pixel's SSIM from its moments about (ca, cb) (m = a', b', a'^2, b'^2, a'b'): luminance ln / ld,
// contrast-structure cn / cd.  No contraction: every expression is evaluated as written, the a and b operands in mirror-image
// positions.
struct PxTerms {
    float ln, ld, cn, cd;
};

__device__ __forceinline__ PxTerms px_terms(const float* m, float ca, float cb, const MetricTaps& t) {
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
    PxTerms p;
    p.ln = 2.f * (ua * ub) + t.c1;
    p.cn = 2.f * sab + t.c2;
    p.ld = (ua * ua + ub * ub) + t.c1;
    p.cd = (saa + sbb) + t.c2;
    return p;
}

// SSIM of one pixel: (ln cn) / (ld cd)
__device__ __forceinline__ float ssim_of(const PxTerms& p) {
#pragma clang fp contract(off)
    const float num = p.ln * p.cn;
    const float den = p.ld * p.cd;
    return num / den;
}

// contrast-structure of one pixel (the multi-scale mode's cs): cn / cd, symmetric in (a, b) and 1 where they agree on the window
__device__ __forceinline__ float cs_of(const PxTerms& p) {
#pragma clang fp contract(off)
    return p.cn / p.cd;
}

__device__ __forceinline__ float ssim_px(const float* m, float ca, float cb, const MetricTaps& t) {
    return ssim_of(px_terms(m, ca, cb, t));
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

// The two passes of one tile, from the halos in sAB (sH: scratch of the horizontal pass): thread (tx = tid & 31, ty = tid >> 5)
// gets the five moments of output pixels (4 ty + o, tx), o = 0 .. 3, about (cenA[o], cenB[o]).  The caller has synchronised
// after writing sAB.
template <int WIN>
__device__ __forceinline__ void tile_moments(const float2* sAB, float* sH, const MetricTaps& taps, int tid, float (&mom)[4][5],
                                             float (&cenA)[4], float (&cenB)[4]) {
    constexpr int R = MT + WIN - 1;   // halo rows / columns
    constexpr int HALF = WIN / 2;
    constexpr int GV = WIN >= 5 ? 4 : 2;   // output rows per vertical group: every one within HALF rows of the centre
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
}

template <int WIN>
__global__ void __launch_bounds__(MTPB) image_metrics_tile_kernel(mmh_image_src A, mmh_image_src Bsrc, int C, int H, int W,
                                                                  int tiles_x, MetricTaps taps, double* __restrict__ part) {
    constexpr int R = MT + WIN - 1;   // halo rows / columns
    constexpr int HALF = WIN / 2;
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

    const int tx = tid & 31, ty = tid >> 5;
    float mom[4][5], cenA[4], cenB[4];
    tile_moments<WIN>(sAB, sH, taps, tid, mom, cenA, cenB);
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

// ---- the two further modes: the same halos, passes and ssim_px; their workgroup reduction lies in sH, which the vertical pass
// has finished with, so neither holds more LDS than the plain kernel

// K sums of one workgroup in the plain kernel's order (lanes of a wave by wave_sum, then the four waves in order) -> p[0 .. K)
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double* sRed, int tid, double* p) {
    __syncthreads();                   // every wave is through with sH
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sRed[(tid >> 6) * K + k] = v[k];
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = sRed[k];
#pragma unroll
            for (int w = 1; w < MTPB / 64; ++w) t += sRed[w * K + k];
            p[k] = t;
        }
    }
}

// Masked mode: per (tile, channel, image) seven partials - the plain kernel's three, the same three over the pixels whose mask
// byte is non-zero (a pixel outside the mask adds 0.0 in its place, so an all-ones mask gives the plain sums' bits), and the
// number of such pixels.
template <int WIN>
__global__ void __launch_bounds__(MTPB) image_metrics_masked_kernel(mmh_image_src A, mmh_image_src Bsrc, const uint8_t* __restrict__ mask,
                                                                    int64_t msb, int64_t msh, int64_t msw, int C, int H, int W,
                                                                    int tiles_x, MetricTaps taps, double* __restrict__ part) {
    constexpr int R = MT + WIN - 1;
    constexpr int HALF = WIN / 2;
    __shared__ float2 sAB[R * MROW];
    __shared__ __attribute__((aligned(16))) float sH[5 * R * HROW];

    const int tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int y0 = (tile / tiles_x) * MT, x0 = (tile % tiles_x) * MT;
    const int tid = threadIdx.x;
    const int tx = tid & 31, ty = tid >> 5;
    const int ox = x0 + tx;
    const int64_t baseA = (int64_t)b * A.sb + (int64_t)c * A.sc;
    const int64_t baseB = (int64_t)b * Bsrc.sb + (int64_t)c * Bsrc.sc;

    // this thread's four mask bytes, in flight under the halo load and the two passes
    bool in[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int oy = y0 + ty * 4 + o;
        in[o] = oy < H && ox < W && mask[(int64_t)b * msb + (int64_t)oy * msh + (int64_t)ox * msw] != 0;
    }
    load_halos<R>(A, baseA, Bsrc, baseB, y0 - HALF, x0 - HALF, H, W, sAB);
    __syncthreads();

    float mom[4][5], cenA[4], cenB[4];
    tile_moments<WIN>(sAB, sH, taps, tid, mom, cenA, cenB);
    double s_ssim = 0.0, s_l1 = 0.0, s_se = 0.0, m_ssim = 0.0, m_l1 = 0.0, m_se = 0.0, m_n = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int oy = y0 + ty * 4 + o;
        if (oy < H && ox < W) {
            const double v = (double)ssim_px(mom[o], cenA[o], cenB[o], taps);
            s_ssim += v;
            const int li = (ty * 4 + o + HALF) * MROW + tx + HALF;
            const double d = (double)sAB[li].x - (double)sAB[li].y;
            s_l1 += fabs(d);
            s_se += d * d;
            const double dm = in[o] ? d : 0.0;      // a product of its own, so both sums are formed by the same instructions
            m_ssim += in[o] ? v : 0.0;
            m_l1 += fabs(dm);
            m_se += dm * dm;
            m_n += in[o] ? 1.0 : 0.0;
        }
    }
    double v[7] = {s_ssim, s_l1, s_se, m_ssim, m_l1, m_se, m_n};
    block_sums<7>(v, reinterpret_cast<double*>(sH), tid, part + (((int64_t)b * C + c) * (int64_t)gridDim.x + tile) * 7);
}

// one workgroup per image: the seven sums over its n partials in the plain final kernel's order.  The count partials of the C
// channels add up to T = C * count exactly; the masked means are sum * (1.0 / T), NaN where the mask is empty.
__global__ void __launch_bounds__(256) image_metrics_masked_final_kernel(const double* __restrict__ part, int n, int C,
                                                                         double inv_count, double* __restrict__ out) {
    __shared__ double sRed[7][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* p = part + (int64_t)b * n * 7;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 7; ++k) s[k] += p[(int64_t)i * 7 + k];
#pragma unroll
    for (int k = 0; k < 7; ++k) sRed[k][tid] = s[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
#pragma unroll
            for (int k = 0; k < 7; ++k) sRed[k][tid] += sRed[k][tid + h];
        __syncthreads();
    }
    const double T = sRed[6][0];
    if (tid < 3) out[(int64_t)b * 7 + tid] = sRed[tid][0] * inv_count;
    else if (tid < 6) out[(int64_t)b * 7 + tid] = T > 0.0 ? sRed[tid][0] * (1.0 / T) : __builtin_nan("");
    else if (tid == 6) out[(int64_t)b * 7 + 6] = T / (double)C;
}

// ((v00 + v01) + (v10 + v11)) * 0.25f as written
__device__ __forceinline__ float pool4(float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    return ((v00 + v01) + (v10 + v11)) * 0.25f;
}

// Multi-scale mode, one level: per (tile, channel, image) two partials - the SSIM map and the contrast-structure map summed
// over the output pixels whose whole window lies inside the image - and, when nextA is given, this tile's 16 x 16 part of the
// next level's pair: pooled pixel (i, j) is the mean of rows 2 i - ph, 2 i - ph + 1 and columns 2 j - pw, 2 j - pw + 1 (ph = H % 2,
// pw = W % 2; zero outside the image, divisor 4).  Row 2 i and column 2 j lie in this tile (its origin is even) and the row or
// column before them in its halo, which is at least one pixel wide.
template <int WIN>
__global__ void __launch_bounds__(MTPB) ms_ssim_level_kernel(mmh_image_src A, mmh_image_src Bsrc, int C, int H, int W, int tiles_x,
                                                             MetricTaps taps, double* __restrict__ part, float* __restrict__ nextA,
                                                             float* __restrict__ nextB) {
    constexpr int R = MT + WIN - 1;
    constexpr int HALF = WIN / 2;
    __shared__ float2 sAB[R * MROW];
    __shared__ __attribute__((aligned(16))) float sH[5 * R * HROW];

    const int tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int y0 = (tile / tiles_x) * MT, x0 = (tile % tiles_x) * MT;
    const int tid = threadIdx.x;
    const int64_t baseA = (int64_t)b * A.sb + (int64_t)c * A.sc;
    const int64_t baseB = (int64_t)b * Bsrc.sb + (int64_t)c * Bsrc.sc;

    load_halos<R>(A, baseA, Bsrc, baseB, y0 - HALF, x0 - HALF, H, W, sAB);
    __syncthreads();

    if (nextA) {
        const int Hn = (H + 1) >> 1, Wn = (W + 1) >> 1;
        const int pi = tid >> 4, pj = tid & 15;
        const int gi = (y0 >> 1) + pi, gj = (x0 >> 1) + pj;
        if (gi < Hn && gj < Wn) {
            const float2* q = sAB + (2 * pi - (H & 1) + HALF) * MROW + (2 * pj - (W & 1) + HALF);
            const float2 v00 = q[0], v01 = q[1], v10 = q[MROW], v11 = q[MROW + 1];
            const int64_t at = (((int64_t)b * C + c) * Hn + gi) * Wn + gj;
            nextA[at] = pool4(v00.x, v01.x, v10.x, v11.x);
            nextB[at] = pool4(v00.y, v01.y, v10.y, v11.y);
        }
    }

    const int tx = tid & 31, ty = tid >> 5;
    float mom[4][5], cenA[4], cenB[4];
    tile_moments<WIN>(sAB, sH, taps, tid, mom, cenA, cenB);
    double s_ssim = 0.0, s_cs = 0.0;
    const int ox = x0 + tx;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int oy = y0 + ty * 4 + o;
        if (oy >= HALF && oy < H - HALF && ox >= HALF && ox < W - HALF) {
            const PxTerms p = px_terms(mom[o], cenA[o], cenB[o], taps);
            s_ssim += (double)ssim_of(p);
            s_cs += (double)cs_of(p);
        }
    }
    double v[2] = {s_ssim, s_cs};
    block_sums<2>(v, reinterpret_cast<double*>(sH), tid, part + (((int64_t)b * C + c) * (int64_t)gridDim.x + tile) * 2);
}

constexpr int MS_MAX_LEVELS = 5;

struct MsPlan {
    int levels;
    int H[MS_MAX_LEVELS], W[MS_MAX_LEVELS], tiles[MS_MAX_LEVELS];
    int64_t part_at[MS_MAX_LEVELS];        // doubles from the workspace's start: level l's [B][C][tiles][2]
    int64_t pyr_at[MS_MAX_LEVELS];         // bytes from the workspace's start: level l's a then b, fp32 [B][C][H_l][W_l] each (l >= 1)
    double inv_count[MS_MAX_LEVELS];       // 1.0 / ((H_l - w + 1)(W_l - w + 1))
    double weight[MS_MAX_LEVELS];
    int64_t bytes;
};

// one workgroup per image: per channel and level the partials of that level in a fixed order (strided per thread, then a fixed
// tree) times 1 / count -> scales; cs for every level but the last, SSIM for the last; out = (sum over c of the product over l of
// pow(max(v, 0), weight)) / C
__global__ void __launch_bounds__(256) ms_ssim_final_kernel(const double* __restrict__ ws, int C, MsPlan plan,
                                                            double* __restrict__ scales, double* __restrict__ out) {
    __shared__ double sRed[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double total = 0.0;
    for (int c = 0; c < C; ++c) {
        double prod = 1.0;
#pragma unroll
        for (int l = 0; l < MS_MAX_LEVELS; ++l) {
            if (l < plan.levels) {
                const int n = plan.tiles[l];
                const double* p = ws + plan.part_at[l] + ((int64_t)b * C + c) * n * 2 + (l == plan.levels - 1 ? 0 : 1);
                double s = 0.0;
                for (int i = tid; i < n; i += 256) s += p[(int64_t)i * 2];
                sRed[tid] = s;
                __syncthreads();
                for (int h = 128; h > 0; h >>= 1) {
                    if (tid < h) sRed[tid] += sRed[tid + h];
                    __syncthreads();
                }
                const double v = sRed[0] * plan.inv_count[l];
                __syncthreads();               // sRed[0] is read before the next level overwrites it
                if (tid == 0) scales[((int64_t)b * C + c) * plan.levels + l] = v;
                prod *= pow(fmax(v, 0.0), plan.weight[l]);
            }
        }
        total += prod;
    }
    if (tid == 0) out[b] = total / (double)C;
}

int64_t metric_tiles(int H, int W) { return mmh::cdiv(H, MT) * mmh::cdiv(W, MT); }

bool metric_shape_ok(int B, int C, int H, int W, int window) {
    return B >= 1 && B <= 65535 && C >= 1 && C <= 65535 && H >= 1 && W >= 1 && window >= 3 && window <= 15 &&
           window % 2 == 1 &&
           // the launch: tiles * 256 work-items in grid dimension x (< 2^32); the final kernel's int count of partials
           metric_tiles(H, W) * MTPB < (int64_t(1) << 32) && (int64_t)C * metric_tiles(H, W) < (int64_t(1) << 31);
}

// f(std::integral_constant<int, window>) for the odd windows 3 .. 15 (the caller has checked the range)
template <typename F>
void with_window(int window, F&& f) {
    switch (window) {
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 9: f(std::integral_constant<int, 9>{}); break;
        case 11: f(std::integral_constant<int, 11>{}); break;
        case 13: f(std::integral_constant<int, 13>{}); break;
        default: f(std::integral_constant<int, 15>{}); break;
    }
}

// the argument checks the three entry points share (fn: the entry point's name in the message)
int check_pair(const char* fn, const mmh_image_src* a, const mmh_image_src* b, int B, int C, int H, int W, int window,
               const float* taps, double c1, double c2, const void* ws, const void* out) {
    MMH_REQUIRE(a && b && a->ptr && b->ptr && ws && out, "%s: NULL argument", fn);
    MMH_REQUIRE(window >= 3 && window <= 15 && window % 2 == 1, "%s: window %d (odd, 3 .. 15)", fn, window);
    MMH_REQUIRE(metric_shape_ok(B, C, H, W, window), "%s: bad shape B=%d C=%d H=%d W=%d", fn, B, C, H, W);
    MMH_REQUIRE(taps && c1 > 0 && c2 > 0, "%s: taps must be given, c1 and c2 > 0", fn);
    double tsum = 0.0;
    for (int i = 0; i < window; ++i) {
        MMH_REQUIRE(taps[i] > 0.f && taps[i] < 1.f, "%s: tap %d = %g (a normalised window has taps in (0, 1))", fn, i, (double)taps[i]);
        tsum += taps[i];
    }
    MMH_REQUIRE(std::fabs(tsum - 1.0) < 1e-5, "%s: the taps sum to %.9g, not 1", fn, tsum);
    for (const mmh_image_src* p : {a, b})
        MMH_REQUIRE(p->dtype == MMH_F32 || p->dtype == MMH_BF16 || p->dtype == MMH_FP16 || p->dtype == MMH_U8, "%s: unknown dtype %d", fn,
                    p->dtype);
    return 0;
}

// the 2-D window is the fp32 outer product of the taps (pytorch_ssim.create_window); its sum, in float64, gives S - 1
MetricTaps metric_taps(int window, const float* taps, double c1, double c2) {
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
    return t;
}

// the multi-scale mode's levels, partial and pyramid offsets; false = the arguments are refused
bool ms_plan(int B, int C, int H, int W, int window, int levels, MsPlan& p) {
    if (!metric_shape_ok(B, C, H, W, window) || levels < 1 || levels > MS_MAX_LEVELS) return false;
    if ((int64_t)std::min(H, W) <= ((int64_t)(window - 1) << (levels - 1))) return false;      // the last level holds a window
    if ((double)B * C * H * W > 1e12) return false;                                            // the pyramid's byte count
    p = MsPlan{};
    p.levels = levels;
    int64_t doubles = 0;
    for (int l = 0; l < levels; ++l) {
        p.H[l] = H;
        p.W[l] = W;
        p.tiles[l] = (int)metric_tiles(H, W);
        p.part_at[l] = doubles;
        doubles += (int64_t)B * C * p.tiles[l] * 2;
        p.inv_count[l] = 1.0 / ((double)(H - window + 1) * (double)(W - window + 1));
        H = (H + 1) / 2;
        W = (W + 1) / 2;
    }
    int64_t bytes = doubles * (int64_t)sizeof(double);
    for (int l = 1; l < levels; ++l) {
        p.pyr_at[l] = bytes;
        bytes += 2 * (int64_t)B * C * p.H[l] * p.W[l] * (int64_t)sizeof(float);
    }
    p.bytes = bytes;
    return true;
}

}  // namespace

size_t mmh_image_metrics_ws_bytes(int B, int C, int H, int W, int window) {
    if (!metric_shape_ok(B, C, H, W, window)) return 0;
    return (size_t)B * C * metric_tiles(H, W) * 3 * sizeof(double);
}

int mmh_image_metrics(const mmh_image_src* a, const mmh_image_src* b, int B, int C, int H, int W, int window, const float* taps,
                      double c1, double c2, void* ws, size_t ws_bytes, double* out, mmh_stream_t s) {
    if (int rc = check_pair("mmh_image_metrics", a, b, B, C, H, W, window, taps, c1, c2, ws, out)) return rc;
    const size_t need = mmh_image_metrics_ws_bytes(B, C, H, W, window);
    MMH_REQUIRE(need > 0 && ws_bytes >= need, "mmh_image_metrics: workspace %zu bytes < %zu", ws_bytes, need);
    const MetricTaps t = metric_taps(window, taps, c1, c2);
    hipStream_t st = mmh::as_stream(s);
    double* part = static_cast<double*>(ws);
    const int tiles_x = (int)mmh::cdiv(W, MT);
    with_window(window, [&](auto w) {
        hipLaunchKernelGGL(image_metrics_tile_kernel<decltype(w)::value>, dim3((unsigned)metric_tiles(H, W), C, B), dim3(MTPB), 0, st,
                           *a, *b, C, H, W, tiles_x, t, part);
    });
    if (int rc = mmh::check_launch("image_metrics_tile")) return rc;
    const int n = (int)(C * metric_tiles(H, W));
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3(B), dim3(256), 0, st, part, n, 1.0 / ((double)C * H * W), out);
    return mmh::check_launch("image_metrics_final");
}

size_t mmh_image_metrics_masked_ws_bytes(int B, int C, int H, int W, int window) {
    if (!metric_shape_ok(B, C, H, W, window)) return 0;
    return (size_t)B * C * metric_tiles(H, W) * 7 * sizeof(double);
}

int mmh_image_metrics_masked(const mmh_image_src* a, const mmh_image_src* b, const uint8_t* mask, int64_t msb, int64_t msh,
                             int64_t msw, int B, int C, int H, int W, int window, const float* taps, double c1, double c2, void* ws,
                             size_t ws_bytes, double* out, mmh_stream_t s) {
    if (int rc = check_pair("mmh_image_metrics_masked", a, b, B, C, H, W, window, taps, c1, c2, ws, out)) return rc;
    MMH_REQUIRE(mask, "mmh_image_metrics_masked: NULL mask");
    const size_t need = mmh_image_metrics_masked_ws_bytes(B, C, H, W, window);
    MMH_REQUIRE(need > 0 && ws_bytes >= need, "mmh_image_metrics_masked: workspace %zu bytes < %zu", ws_bytes, need);
    const MetricTaps t = metric_taps(window, taps, c1, c2);
    hipStream_t st = mmh::as_stream(s);
    double* part = static_cast<double*>(ws);
    const int tiles_x = (int)mmh::cdiv(W, MT);
    with_window(window, [&](auto w) {
        hipLaunchKernelGGL(image_metrics_masked_kernel<decltype(w)::value>, dim3((unsigned)metric_tiles(H, W), C, B), dim3(MTPB), 0,
                           st, *a, *b, mask, msb, msh, msw, C, H, W, tiles_x, t, part);
    });
    if (int rc = mmh::check_launch("image_metrics_masked")) return rc;
    const int n = (int)(C * metric_tiles(H, W));
    hipLaunchKernelGGL(image_metrics_masked_final_kernel, dim3(B), dim3(256), 0, st, part, n, C, 1.0 / ((double)C * H * W), out);
    return mmh::check_launch("image_metrics_masked_final");
}

size_t mmh_ms_ssim_ws_bytes(int B, int C, int H, int W, int window, int levels) {
    MsPlan p;
    return ms_plan(B, C, H, W, window, levels, p) ? (size_t)p.bytes : 0;
}

int mmh_ms_ssim(const mmh_image_src* a, const mmh_image_src* b, int B, int C, int H, int W, int window, const float* taps, double c1,
                double c2, int levels, const double* weights, void* ws, size_t ws_bytes, double* scales, double* out,
                mmh_stream_t s) {
    if (int rc = check_pair("mmh_ms_ssim", a, b, B, C, H, W, window, taps, c1, c2, ws, out)) return rc;
    MMH_REQUIRE(scales && weights, "mmh_ms_ssim: NULL argument");
    MMH_REQUIRE(levels >= 1 && levels <= MS_MAX_LEVELS, "mmh_ms_ssim: levels %d (1 .. %d)", levels, MS_MAX_LEVELS);
    MsPlan plan;
    MMH_REQUIRE(ms_plan(B, C, H, W, window, levels, plan),
                "mmh_ms_ssim: bad shape H=%d W=%d: min(H, W) must exceed (window - 1) * 2^(levels - 1) = %d", H, W,
                (window - 1) << (levels - 1));
    for (int l = 0; l < levels; ++l) {
        MMH_REQUIRE(weights[l] > 0.0 && std::isfinite(weights[l]), "mmh_ms_ssim: weight %d = %g (finite, > 0)", l, weights[l]);
        plan.weight[l] = weights[l];
    }
    MMH_REQUIRE(ws_bytes >= (size_t)plan.bytes, "mmh_ms_ssim: workspace %zu bytes < %zu", ws_bytes, (size_t)plan.bytes);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "mmh_ms_ssim: the workspace must be 8-byte aligned");
    const MetricTaps t = metric_taps(window, taps, c1, c2);
    hipStream_t st = mmh::as_stream(s);
    double* part = static_cast<double*>(ws);
    mmh_image_src la = *a, lb = *b;
    for (int l = 0; l < levels; ++l) {
        const int Hl = plan.H[l], Wl = plan.W[l];
        float *na = nullptr, *nb = nullptr;
        int64_t plane = 0;
        if (l + 1 < levels) {       // the next level's pair, written by this level's launch
            plane = (int64_t)plan.H[l + 1] * plan.W[l + 1];
            na = reinterpret_cast<float*>(static_cast<char*>(ws) + plan.pyr_at[l + 1]);
            nb = na + (int64_t)B * C * plane;
        }
        const int tiles_x = (int)mmh::cdiv(Wl, MT);
        with_window(window, [&](auto w) {
            hipLaunchKernelGGL(ms_ssim_level_kernel<decltype(w)::value>, dim3((unsigned)plan.tiles[l], C, B), dim3(MTPB), 0, st, la, lb,
                               C, Hl, Wl, tiles_x, t, part + plan.part_at[l], na, nb);
        });
        if (int rc = mmh::check_launch("ms_ssim_level")) return rc;
        if (na) {
            la = mmh_image_src{na, MMH_F32, 1.f, 0.f, C * plane, plane, plan.W[l + 1], 1};
            lb = mmh_image_src{nb, MMH_F32, 1.f, 0.f, C * plane, plane, plan.W[l + 1], 1};
        }
    }
    hipLaunchKernelGGL(ms_ssim_final_kernel, dim3(B), dim3(256), 0, st, part, C, plan, scales, out);
    return mmh::check_launch("ms_ssim_final");
}


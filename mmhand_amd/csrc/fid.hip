// The two reductions behind the Frechet Inception Distance and the Kernel Inception Distance over pooled Inception features
// (fp32 [N][d], d = 2048 in use), for gfx950.  Definitions: pytorch-fid (mu, np.cov(rowvar=False)) and torch-fidelity's KID
// (kernel (x.y / d + 1)^3, unbiased MMD^2 over subsets).  Both are all-pairs products on the fp64 MFMA
// (v_mfma_f64_16x16x4_f64) whose results never lie in memory as a matrix of pairs (KID) or are written once (covariance).
//
// A workgroup of four waves owns one 64 x 64 output tile; wave (wi, wj) owns its 32 x 32 quadrant as 2 x 2 MFMA tiles.  The
// summed dimension - the N rows for the covariance, the d features for the kernel - is long, so the operands are staged
// through LDS in blocks as float64 (fp32 -> fp64 is exact, and so is the product of two converted values: the accumulation is
// the only rounding).  While a block is multiplied the next one is already on its way in registers.  Every output element is
// ONE chain of MFMAs over the summed dimension in ascending order, from a zero accumulator, whatever tile, wave or lane it
// falls in: its bits depend on the operand values alone.  The fp64 C/D lane map is col = lane & 15, rows (lane >> 4) + 4 reg
// (pose_knn.hip's, not the f32 map); A and B hold one value per lane, index lane & 15 along the tile, lane >> 4 along k.
//
// LDS images and their bank behaviour (ds_read_b64: banks (byte / 4) mod 64, conflicts inside each 32-lane half):
//   covariance  [32 rows of X][80]  - a half wave reads 16 consecutive doubles of two rows: 160 dwords apart = 32 mod 64.
//   kernel      [64 rows][34]       - a half wave reads features f, f + 1 of 16 rows 68 dwords apart = 4 mod 64.
// Both are conflict-free.  40 KiB and 34 KiB per workgroup: three to four workgroups per CU hide each other's barriers.
//
// Only tiles on or above the diagonal of a symmetric result are multiplied (a workgroup below it returns at once).  No atomics,
// no spin waits; every sum has an order fixed by the shapes, so two runs give the same bits.
#include "common.h"

namespace {

constexpr int FT = 64;            // output tile edge
constexpr int FTPB = 256;         // 4 waves, 2 x 2 quadrants
constexpr int CKB = 32;           // covariance: rows of X per LDS block
constexpr int CSK = 80;           // ... and the row stride of its image, in doubles
constexpr int MCH = 128;          // column means: rows per partial sum
constexpr int KKF = 32;           // kernel sums: features per LDS block
constexpr int KSC = 34;           // ... and the row stride of its image, in doubles
constexpr int RTPB = 256;         // the tile-sum reduction's workgroup

typedef double double4_t __attribute__((ext_vector_type(4)));

// ksteps MFMA steps of a wave's 2 x 2 tiles; element (k, i) of an image lies at k * SK + i * SC
template <int SK, int SC>
__device__ __forceinline__ void tile_mma(const double* __restrict__ sI, const double* __restrict__ sJ, int ksteps, int wi, int wj,
                                         int lane, double4_t (&acc)[2][2]) {
    const double* pi = sI + (lane >> 4) * SK + (wi * 32 + (lane & 15)) * SC;
    const double* pj = sJ + (lane >> 4) * SK + (wj * 32 + (lane & 15)) * SC;
    for (int s = 0; s < ksteps; ++s) {
        const double a0 = pi[s * 4 * SK], a1 = pi[s * 4 * SK + 16 * SC];
        const double b0 = pj[s * 4 * SK], b1 = pj[s * 4 * SK + 16 * SC];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ float4 ld4_or_zero(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------- moments
// pass 1a: thread = (column, chunk of MCH rows): the chunk's rows in order
__global__ void __launch_bounds__(256) fid_colsum_kernel(const float* __restrict__ X, int N, int d, double* __restrict__ part) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    const int n0 = blockIdx.y * MCH, n1 = n0 + MCH < N ? n0 + MCH : N;
    double s = 0.0;
    for (int n = n0; n < n1; ++n) s += (double)X[(int64_t)n * d + col];
    part[(int64_t)blockIdx.y * d + col] = s;
}

// pass 1b: thread = column: the chunks in order, divided once
__global__ void __launch_bounds__(256) fid_mean_kernel(const double* __restrict__ part, int chunks, int N, int d,
                                                       double* __restrict__ mean) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * d + col];
    mean[col] = s / (double)N;
}

// pass 2: tile (bi, bj), bi <= bj, of sum_n c[n][i] c[n][j] / (N - 1), c = (double)x - mean, and its mirror
__global__ void __launch_bounds__(FTPB) fid_cov_kernel(const float* __restrict__ X, int N, int d, const double* __restrict__ mean,
                                                       double* __restrict__ cov) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ double sI[CKB * CSK];
    __shared__ double sJ[CKB * CSK];
    const bool diag = bi == bj;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wi = wave >> 1, wj = wave & 1;
    // staging: thread = (row r0 and r0 + 16 of the block, column quad c4); d % 4 == 0, so a quad is inside or outside as a whole
    const int c4 = tid & 15, r0 = tid >> 4;
    const int ci = bi * FT + c4 * 4, cj = bj * FT + c4 * 4;
    const bool okI = ci < d, okJ = !diag && cj < d;
    double mI[4], mJ[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mI[e] = okI ? mean[ci + e] : 0.0;
        mJ[e] = okJ ? mean[cj + e] : 0.0;
    }
    float4 vI[2], vJ[2];
    auto fetch = [&](int n0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n0 + r0 + 16 * h;
            vI[h] = ld4_or_zero(X + (int64_t)n * d + ci, okI && n < N);
            vJ[h] = ld4_or_zero(X + (int64_t)n * d + cj, okJ && n < N);
        }
    };
    auto stash = [&](int n0) {          // a row past N and a column past d hold zeros: their products add nothing
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool in = n0 + r0 + 16 * h < N;
            double* p = sI + (r0 + 16 * h) * CSK + c4 * 4;
            const bool a = in && okI;
            p[0] = a ? (double)vI[h].x - mI[0] : 0.0;
            p[1] = a ? (double)vI[h].y - mI[1] : 0.0;
            p[2] = a ? (double)vI[h].z - mI[2] : 0.0;
            p[3] = a ? (double)vI[h].w - mI[3] : 0.0;
            if (!diag) {
                double* q = sJ + (r0 + 16 * h) * CSK + c4 * 4;
                const bool b = in && okJ;
                q[0] = b ? (double)vJ[h].x - mJ[0] : 0.0;
                q[1] = b ? (double)vJ[h].y - mJ[1] : 0.0;
                q[2] = b ? (double)vJ[h].z - mJ[2] : 0.0;
                q[3] = b ? (double)vJ[h].w - mJ[3] : 0.0;
            }
        }
    };
    double4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    const double* pJ = diag ? sI : sJ;          // a diagonal tile: both operands from the same block
    fetch(0);
    for (int n0 = 0; n0 < N; n0 += CKB) {
        stash(n0);
        __syncthreads();
        if (n0 + CKB < N) fetch(n0 + CKB);
        const int rows = N - n0 < CKB ? N - n0 : CKB;
        tile_mma<CSK, 1>(sI, pJ, (rows + 3) / 4, wi, wj, lane, acc);
        __syncthreads();
    }
    const double denom = (double)(N - 1);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = bi * FT + wi * 32 + a * 16 + (lane >> 4) + 4 * r;
                const int j = bj * FT + wj * 32 + b * 16 + (lane & 15);
                if (i < d && j < d && i <= j) {
                    const double v = acc[a][b][r] / denom;
                    cov[(int64_t)i * d + j] = v;
                    cov[(int64_t)j * d + i] = v;
                }
            }
}

// ------------------------------------------------------------------------------------------------- kernel sums
// The tiles of a subset, in this order: A x A (TA x TA), B x B (TB x TB), A x B (TA x TB), each row-major; a tile below the
// diagonal of the two symmetric blocks is never computed and never read.
struct MmdTile {
    int which, bi, bj, cols;
};

__device__ __forceinline__ MmdTile mmd_tile(int t, int TA, int TB) {
    MmdTile m;
    if (t < TA * TA) {
        m.which = 0; m.cols = TA;
    } else if (t < TA * TA + TB * TB) {
        t -= TA * TA; m.which = 1; m.cols = TB;
    } else {
        t -= TA * TA + TB * TB; m.which = 2; m.cols = TB;
    }
    m.bi = t / m.cols;
    m.bj = t % m.cols;
    return m;
}

__global__ void __launch_bounds__(FTPB) fid_mmd_tile_kernel(const float* __restrict__ A, const float* __restrict__ B, int d,
                                                            const int32_t* __restrict__ idxA, const int32_t* __restrict__ idxB,
                                                            int Ma, int Mb, int TA, int TB, int64_t ntiles, double* __restrict__ ws) {
#pragma clang fp contract(off)
    const MmdTile m = mmd_tile(blockIdx.x, TA, TB);
    const bool sym = m.which < 2;
    if (sym && m.bi > m.bj) return;
    __shared__ double sI[FT * KSC];
    __shared__ double sJ[FT * KSC];
    __shared__ double sW[FTPB / 64];
    const int s = blockIdx.y;
    const float* P = m.which == 1 ? B : A;
    const float* Q = m.which == 0 ? A : B;
    const int Mi = m.which == 1 ? Mb : Ma, Mj = m.which == 0 ? Ma : Mb;
    const int32_t* ip = m.which == 1 ? idxB + (int64_t)s * Mb : idxA + (int64_t)s * Ma;
    const int32_t* iq = m.which == 0 ? idxA + (int64_t)s * Ma : idxB + (int64_t)s * Mb;
    const bool diag = sym && m.bi == m.bj;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wi = wave >> 1, wj = wave & 1;
    // staging: thread = (list positions row and row + 32 of the tile, feature quad f4 of the block)
    const int f4 = tid & 7, row = tid >> 3;
    int64_t rI[2], rJ[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = m.bi * FT + row + 32 * h, q = m.bj * FT + row + 32 * h;
        rI[h] = p < Mi ? (int64_t)ip[p] : -1;
        rJ[h] = (!diag && q < Mj) ? (int64_t)iq[q] : -1;
    }
    float4 vI[2], vJ[2];
    auto fetch = [&](int f0) {
        const int f = f0 + 4 * f4;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            vI[h] = ld4_or_zero(P + rI[h] * d + f, rI[h] >= 0 && f < d);
            vJ[h] = ld4_or_zero(Q + rJ[h] * d + f, rJ[h] >= 0 && f < d);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double* p = sI + (row + 32 * h) * KSC + 4 * f4;
            p[0] = (double)vI[h].x; p[1] = (double)vI[h].y; p[2] = (double)vI[h].z; p[3] = (double)vI[h].w;
            if (!diag) {
                double* q = sJ + (row + 32 * h) * KSC + 4 * f4;
                q[0] = (double)vJ[h].x; q[1] = (double)vJ[h].y; q[2] = (double)vJ[h].z; q[3] = (double)vJ[h].w;
            }
        }
    };
    double4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    const double* pJ = diag ? sI : sJ;
    fetch(0);
    for (int f0 = 0; f0 < d; f0 += KKF) {
        stash();
        __syncthreads();
        if (f0 + KKF < d) fetch(f0 + KKF);
        const int feats = d - f0 < KKF ? d - f0 : KKF;          // d % 4 == 0: exactly d / 4 MFMAs in all
        tile_mma<1, KSC>(sI, pJ, feats / 4, wi, wj, lane, acc);
        __syncthreads();
    }
    // k = ((t t) t), t = dot / d + 1; the lane's 16 values in (a, b, r) order, then a butterfly, then the four waves in order
    const double dd = (double)d;
    double lsum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = m.bi * FT + wi * 32 + a * 16 + (lane >> 4) + 4 * r;
                const int q = m.bj * FT + wj * 32 + b * 16 + (lane & 15);
                if (p < Mi && q < Mj && !(sym && p == q)) {
                    const double t = acc[a][b][r] / dd + 1.0;
                    const double k = (t * t) * t;
                    lsum = lsum + k;
                }
            }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lsum = lsum + __shfl_xor(lsum, off);
    if (lane == 0) sW[wave] = lsum;
    __syncthreads();
    if (tid == 0) ws[(int64_t)s * ntiles + blockIdx.x] = ((sW[0] + sW[1]) + sW[2]) + sW[3];
}

// workgroup = (sum 0 | 1 | 2, subset): thread i adds tiles i, i + 256, ... of the block in tile order (a tile above the
// diagonal of a symmetric block counts twice - exact), then a fixed pairwise tree over the 256 partial sums
__global__ void __launch_bounds__(RTPB) fid_mmd_sum_kernel(const double* __restrict__ ws, int TA, int TB, int64_t ntiles,
                                                           double* __restrict__ out) {
    __shared__ double sP[RTPB];
    const int which = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int base = which == 0 ? 0 : (which == 1 ? TA * TA : TA * TA + TB * TB);
    const int rows = which == 1 ? TB : TA, cols = which == 0 ? TA : TB;
    const double* w = ws + (int64_t)s * ntiles + base;
    double part = 0.0;
    for (int t = tid; t < rows * cols; t += RTPB) {
        const int bi = t / cols, bj = t % cols;
        if (which < 2 && bi > bj) continue;
        const double v = w[t];
        part += (which < 2 && bi < bj) ? 2.0 * v : v;
    }
    sP[tid] = part;
    __syncthreads();
    for (int n = RTPB / 2; n >= 1; n >>= 1) {
        if (tid < n) sP[tid] = sP[tid] + sP[tid + n];
        __syncthreads();
    }
    if (tid == 0) out[(int64_t)s * 3 + which] = sP[0];
}

bool mmd_plan(int S, int Ma, int Mb, int* TA, int* TB, int64_t* ntiles) {
    if (S < 1 || S > 65535 || Ma < 1 || Mb < 1) return false;
    const int64_t ta = mmh::cdiv(Ma, FT), tb = mmh::cdiv(Mb, FT);
    const int64_t n = ta * ta + tb * tb + ta * tb;
    if (n >= (int64_t(1) << 31)) return false;
    *TA = (int)ta;
    *TB = (int)tb;
    *ntiles = n;
    return true;
}

bool moments_ok(int N, int d) {
    return N >= 2 && d >= 4 && d % 4 == 0 && mmh::cdiv(d, FT) <= 65535 && mmh::cdiv(N, MCH) <= 65535;
}

}  // namespace

size_t mmh_feature_moments_ws_bytes(int N, int d) {
    if (!moments_ok(N, d)) return 0;
    return ((size_t)mmh::cdiv(N, MCH) * (size_t)d * 8 + 255) / 256 * 256;
}

int mmh_feature_moments(const float* X, int N, int d, double* mean, double* cov, void* ws, mmh_stream_t s) {
    MMH_REQUIRE(X && mean && cov && ws, "mmh_feature_moments (fid): NULL argument");
    MMH_REQUIRE(moments_ok(N, d), "mmh_feature_moments (fid): N = %d, d = %d (N >= 2 rows, d a multiple of 4)", N, d);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(cov) |
                                                                 reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "mmh_feature_moments (fid): X must be 16-byte aligned, mean, cov and the workspace 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    const int chunks = (int)mmh::cdiv(N, MCH);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(fid_colsum_kernel, dim3((unsigned)mmh::cdiv(d, 256), chunks), dim3(256), 0, st, X, N, d, part);
    if (int rc = mmh::check_launch("fid_colsum")) return rc;
    hipLaunchKernelGGL(fid_mean_kernel, dim3((unsigned)mmh::cdiv(d, 256)), dim3(256), 0, st, part, chunks, N, d, mean);
    if (int rc = mmh::check_launch("fid_mean")) return rc;
    const unsigned tiles = (unsigned)mmh::cdiv(d, FT);
    hipLaunchKernelGGL(fid_cov_kernel, dim3(tiles, tiles), dim3(FTPB), 0, st, X, N, d, mean, cov);
    return mmh::check_launch("fid_cov");
}

size_t mmh_poly_mmd_sums_ws_bytes(int S, int Ma, int Mb) {
    int TA, TB;
    int64_t ntiles;
    if (!mmd_plan(S, Ma, Mb, &TA, &TB, &ntiles)) return 0;
    return ((size_t)S * (size_t)ntiles * 8 + 255) / 256 * 256;
}

int mmh_poly_mmd_sums(const float* A, const float* B, int d, const int32_t* idxA, const int32_t* idxB, int S, int Ma, int Mb,
                      double* out, void* ws, mmh_stream_t s) {
    MMH_REQUIRE(A && B && idxA && idxB && out && ws, "mmh_poly_mmd_sums (fid): NULL argument");
    MMH_REQUIRE(d >= 4 && d % 4 == 0, "mmh_poly_mmd_sums (fid): d = %d (a multiple of 4)", d);
    int TA, TB;
    int64_t ntiles;
    MMH_REQUIRE(mmd_plan(S, Ma, Mb, &TA, &TB, &ntiles), "mmh_poly_mmd_sums (fid): S = %d, Ma = %d, Mb = %d (1 .. 65535 subsets of at least "
                "one row each, fewer than 2^31 tiles)", S, Ma, Mb);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 &&
                    ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "mmh_poly_mmd_sums (fid): A and B must be 16-byte aligned, out and the workspace 8-byte aligned");
    hipStream_t st = mmh::as_stream(s);
    double* w = static_cast<double*>(ws);
    hipLaunchKernelGGL(fid_mmd_tile_kernel, dim3((unsigned)ntiles, S), dim3(FTPB), 0, st, A, B, d, idxA, idxB, Ma, Mb, TA, TB, ntiles, w);
    if (int rc = mmh::check_launch("fid_mmd_tile")) return rc;
    hipLaunchKernelGGL(fid_mmd_sum_kernel, dim3(3, S), dim3(RTPB), 0, st, w, TA, TB, ntiles, out);
    return mmh::check_launch("fid_mmd_sum");
}

// Pose distance of the reference (nearest_neighbor_search/nearest_neighbor_search.py:68-83, poseDistance) for gfx950, and the
// exact k nearest candidates of every query under it - the quantity behind curriculum training and nearest-source match.
//
//   feature(pose) = the 20 consecutive joint differences C[i] - C[i-1] (60 values) divided by their float64 2-norm, padded
//                   with 4 zeros to 64;   cos(u, v) = feature(u) . feature(v);   d = arccos(clamp(cos, -1, 1)) / pi.
// The clamp is a stated divergence: the reference returns NaN where rounding puts the cosine above 1 (identical poses).
//
// pose_knn_slice_kernel: all-pairs cosines on the fp64 MFMA (v_mfma_f64_16x16x4_f64) with a selection epilogue - the
// Nq x Nc matrix never exists.  Queries sit on the columns of the 16 x 16 tile, candidates on its rows, so a lane
// (col = lane & 15, rows (lane >> 4) + 4 reg - the f64 C/D map, NOT the f32 one) only ever sees results of ITS query and
// keeps that query's best k in registers (pose_topk.h).  A workgroup owns 32 queries (two column groups per wave, their
// operands resident in registers) and one slice of the candidates; its four waves take the slice's 16-row tiles in turn.
// At the end the 4 lane groups x 4 waves hand their lists through LDS to one thread per query, which writes the slice's
// best k to the workspace.  pose_knn_merge_kernel merges the slices of a query in slice order and applies arccos.
//
// Every cosine is ONE chain of 16 MFMAs over the same operand values wherever its tile lies (step s multiplies the features
// s, 16 + s, 32 + s, 48 + s - lane group g holds features 16 g .. 16 g + 15 of its row, one 128-byte run), and selection
// is by a total order (larger cosine, then smaller index): the result is bit-identical for any slicing.  No atomics, no
// spin waits; the two kernels are ordered by the stream.
#include <cmath>
#include "common.h"
#include "pose_topk.h"

namespace {

constexpr int PF = 64;            // feature row: 60 values + 4 zeros
constexpr int PQB = 32;           // queries per workgroup: 2 column groups of 16
constexpr int PQG = PQB / 16;
constexpr int PTPB = 256;         // 4 waves
constexpr int PWAVES = PTPB / 64;
constexpr int PMAX_AUTO_SLICES = 32;

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) pose_features_kernel(const double* __restrict__ C, int N, double* __restrict__ F,
                                                            int32_t* __restrict__ valid) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const double* p = C + (int64_t)n * 63;
    double* f = F + (int64_t)n * PF;
    bool finite = true;
    double ss = 0.0;
    for (int j = 0; j < 60; ++j) {
        const double a = p[j], b = p[j + 3];
        finite = finite && __builtin_isfinite(a) && __builtin_isfinite(b);
        const double d = b - a;
        ss += d * d;
    }
    const double nrm = sqrt(ss);
    const bool ok = finite && nrm > 0.0 && __builtin_isfinite(nrm);
    for (int j = 0; j < 60; ++j) f[j] = ok ? (p[j + 3] - p[j]) / nrm : 0.0;
    for (int j = 60; j < PF; ++j) f[j] = 0.0;
    valid[n] = ok ? 1 : 0;
}

// lane group g's 16 features of row `row` (zeros for a row outside [0, n))
__device__ __forceinline__ void load_frag(const double* __restrict__ F, int64_t row, bool inside, int g, double* v) {
    if (inside) {
        const double2* p = reinterpret_cast<const double2*>(F + row * PF + g * 16);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const double2 t = p[s];
            v[2 * s] = t.x;
            v[2 * s + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = 0.0;
    }
}

template <int KT>
__global__ void __launch_bounds__(PTPB) pose_knn_slice_kernel(const double* __restrict__ Fq, int Nq, const double* __restrict__ Fc,
                                                              const int32_t* __restrict__ validc, int Nc,
                                                              const int32_t* __restrict__ exclude, int k, int64_t per,
                                                              double* __restrict__ ws_cos, int32_t* __restrict__ ws_idx) {
    __shared__ double sC[KT * 4 * PQB];
    __shared__ int32_t sI[KT * 4 * PQB];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, g = lane >> 4;
    const int slice = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * PQB;

    // the queries' operands (B: k = lane >> 4, column = lane & 15), resident for the whole slice
    double b[PQG][16];
    int32_t excl[PQG];
#pragma unroll
    for (int t = 0; t < PQG; ++t) {
        const int64_t q = q0 + t * 16 + col;
        load_frag(Fq, q, q < Nq, g, b[t]);
        excl[t] = (exclude != nullptr && q < Nq) ? exclude[q] : -1;
    }
    PoseTopK<KT> top[PQG];
#pragma unroll
    for (int t = 0; t < PQG; ++t) top[t].clear();

    const int64_t c_begin = slice * per;
    const int64_t c_end = c_begin + per < Nc ? c_begin + per : (int64_t)Nc;
    double a[16], an[16];
    int64_t c0 = c_begin + wave * 16;
    if (c0 < c_end) load_frag(Fc, c0 + col, c0 + col < c_end, g, a);
    for (; c0 < c_end; c0 += PWAVES * 16) {
        // the next tile's candidate rows are requested before this tile's products start
        const int64_t cn = c0 + PWAVES * 16;
        if (cn < c_end) load_frag(Fc, cn + col, cn + col < c_end, g, an);
        // this lane's four result rows: candidates c0 + g + 4 r
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t c = c0 + g + 4 * r;
            ok[r] = c < c_end && validc[c] != 0;
        }
        double4_t acc[PQG];
#pragma unroll
        for (int t = 0; t < PQG; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int t = 0; t < PQG; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t][s], acc[t], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int32_t c = (int32_t)(c0 + g + 4 * r);
#pragma unroll
            for (int t = 0; t < PQG; ++t)
                if (ok[r] && c != excl[t]) top[t].insert(acc[t][r], c);
        }
        if (cn < c_end) {
#pragma unroll
            for (int s = 0; s < 16; ++s) a[s] = an[s];
        }
    }

    // 16 lists per query (4 lane groups x 4 waves) -> one: a wave at a time through LDS, thread ql < 32 owns query q0 + ql
    PoseTopK<KT> fin;
    fin.clear();
    for (int w = 0; w < PWAVES; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < PQG; ++t)
#pragma unroll
                for (int j = 0; j < KT; ++j) {
                    sC[(j * 4 + g) * PQB + t * 16 + col] = top[t].c[j];
                    sI[(j * 4 + g) * PQB + t * 16 + col] = top[t].i[j];
                }
        }
        __syncthreads();
        if (tid < PQB) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) fin.merge(sC + gg * PQB + tid, sI + gg * PQB + tid, KT, 4 * PQB);
        }
    }
    if (tid < PQB && q0 + tid < Nq) {
        const int64_t o = ((int64_t)slice * Nq + q0 + tid) * k;
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < k) {
                ws_cos[o + j] = fin.c[j];
                ws_idx[o + j] = fin.i[j];
            }
    }
}

__device__ __forceinline__ double pose_dist_of_cos(double c) {
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    return acos(c) / 3.14159265358979323846;
}

// one thread per query: its slices' lists in slice order -> idx, dist
template <int KT>
__global__ void __launch_bounds__(256) pose_knn_merge_kernel(const double* __restrict__ ws_cos, const int32_t* __restrict__ ws_idx,
                                                             const int32_t* __restrict__ validq, int Nq, int k, int slices,
                                                             int32_t* __restrict__ idx, double* __restrict__ dist) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= Nq) return;
    PoseTopK<KT> fin;
    fin.clear();
    if (validq[q] != 0)
        for (int s = 0; s < slices; ++s) {
            const int64_t o = ((int64_t)s * Nq + q) * k;
            fin.merge(ws_cos + o, ws_idx + o, k, 1);
        }
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j < k) {
            const bool empty = fin.i[j] == POSE_TOPK_EMPTY;
            idx[q * k + j] = empty ? -1 : fin.i[j];
            dist[q * k + j] = empty ? __builtin_nan("") : pose_dist_of_cos(fin.c[j]);
        }
}

__global__ void __launch_bounds__(256) pose_pair_distance_kernel(const double* __restrict__ Fa, const int32_t* __restrict__ va,
                                                                 const double* __restrict__ Fb, const int32_t* __restrict__ vb,
                                                                 int n, double* __restrict__ d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (va[i] == 0 || vb[i] == 0) {
        d[i] = __builtin_nan("");
        return;
    }
    const double* a = Fa + (int64_t)i * PF;
    const double* b = Fb + (int64_t)i * PF;
    double s = 0.0;
    for (int j = 0; j < PF; ++j) s = __builtin_fma(a[j], b[j], s);
    d[i] = pose_dist_of_cos(s);
}

struct PosePlan {
    int64_t per;
    int slices;
};

bool pose_plan(int Nq, int Nc, int k, int cand_split, PosePlan* p) {
    if (Nq < 1 || Nc < 1 || k < 1 || k > POSE_TOPK_MAX || cand_split < 0 || cand_split % 16 != 0) return false;
    int64_t per = cand_split;
    if (cand_split == 0) {
        // enough workgroups for the device (256 CUs, a few each) while a slice keeps every wave a few tiles
        const int64_t qblocks = mmh::cdiv(Nq, PQB);
        int64_t want = mmh::cdiv(1024, qblocks);
        want = want < 1 ? 1 : (want > PMAX_AUTO_SLICES ? PMAX_AUTO_SLICES : want);
        per = mmh::cdiv(mmh::cdiv(Nc, want), 16) * 16;
        if (per < PWAVES * 16) per = PWAVES * 16;
    }
    const int64_t slices = mmh::cdiv(Nc, per);
    if (slices > 65535) return false;
    p->per = per;
    p->slices = (int)slices;
    return true;
}

template <int KT>
int pose_knn_launch(const double* Fq, const int32_t* validq, int Nq, const double* Fc, const int32_t* validc, int Nc,
                    const int32_t* exclude, int k, const PosePlan& p, double* ws_cos, int32_t* ws_idx, int32_t* idx, double* dist,
                    hipStream_t st) {
    hipLaunchKernelGGL(pose_knn_slice_kernel<KT>, dim3((unsigned)mmh::cdiv(Nq, PQB), p.slices), dim3(PTPB), 0, st, Fq, Nq, Fc, validc,
                       Nc, exclude, k, p.per, ws_cos, ws_idx);
    if (int rc = mmh::check_launch("pose_knn_slice")) return rc;
    hipLaunchKernelGGL(pose_knn_merge_kernel<KT>, dim3((unsigned)mmh::cdiv(Nq, 256)), dim3(256), 0, st, ws_cos, ws_idx, validq, Nq, k,
                       p.slices, idx, dist);
    return mmh::check_launch("pose_knn_merge");
}

}  // namespace

int mmh_pose_features(const double* C, int N, double* F, int32_t* valid, mmh_stream_t s) {
    MMH_REQUIRE(C && F && valid, "mmh_pose_features (pose_knn): NULL argument");
    MMH_REQUIRE(N >= 1, "mmh_pose_features (pose_knn): N = %d (at least 1 pose)", N);
    hipLaunchKernelGGL(pose_features_kernel, dim3((unsigned)mmh::cdiv(N, 256)), dim3(256), 0, mmh::as_stream(s), C, N, F, valid);
    return mmh::check_launch("pose_features");
}

size_t mmh_pose_knn_ws_bytes(int Nq, int Nc, int k, int cand_split) {
    PosePlan p;
    if (!pose_plan(Nq, Nc, k, cand_split, &p)) return 0;
    const size_t n = (size_t)p.slices * (size_t)Nq * (size_t)k;     // 8 bytes of cosine + 4 of index each
    return (n * 12 + 255) / 256 * 256;
}

int mmh_pose_knn(const double* Fq, const int32_t* validq, int Nq, const double* Fc, const int32_t* validc, int Nc,
                 const int32_t* exclude, int k, int cand_split, void* ws, int32_t* idx, double* dist, mmh_stream_t s) {
    MMH_REQUIRE(Fq && validq && Fc && validc && ws && idx && dist, "mmh_pose_knn (pose_knn): NULL argument");
    MMH_REQUIRE(Nq >= 1 && Nc >= 1, "mmh_pose_knn (pose_knn): Nq = %d, Nc = %d (at least 1 each)", Nq, Nc);
    MMH_REQUIRE(k >= 1 && k <= POSE_TOPK_MAX, "mmh_pose_knn (pose_knn): k = %d (1 .. %d)", k, POSE_TOPK_MAX);
    MMH_REQUIRE(cand_split >= 0 && cand_split % 16 == 0,
                "mmh_pose_knn (pose_knn): cand_split = %d (0 = automatic, else candidates per slice, a multiple of 16)", cand_split);
    MMH_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(Fq) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(Fc) & 15) == 0,
                "mmh_pose_knn (pose_knn): the workspace must be 8-byte aligned, the feature arrays 16-byte aligned");
    PosePlan p;
    MMH_REQUIRE(pose_plan(Nq, Nc, k, cand_split, &p), "mmh_pose_knn (pose_knn): cand_split = %d cuts %d candidates into more than 65535 slices",
                cand_split, Nc);
    double* ws_cos = static_cast<double*>(ws);
    int32_t* ws_idx = reinterpret_cast<int32_t*>(ws_cos + (size_t)p.slices * (size_t)Nq * (size_t)k);
    hipStream_t st = mmh::as_stream(s);
    switch (pose_topk_size(k)) {
        case 1: return pose_knn_launch<1>(Fq, validq, Nq, Fc, validc, Nc, exclude, k, p, ws_cos, ws_idx, idx, dist, st);
        case 2: return pose_knn_launch<2>(Fq, validq, Nq, Fc, validc, Nc, exclude, k, p, ws_cos, ws_idx, idx, dist, st);
        case 4: return pose_knn_launch<4>(Fq, validq, Nq, Fc, validc, Nc, exclude, k, p, ws_cos, ws_idx, idx, dist, st);
        case 8: return pose_knn_launch<8>(Fq, validq, Nq, Fc, validc, Nc, exclude, k, p, ws_cos, ws_idx, idx, dist, st);
        default: return pose_knn_launch<16>(Fq, validq, Nq, Fc, validc, Nc, exclude, k, p, ws_cos, ws_idx, idx, dist, st);
    }
}

int mmh_pose_pair_distance(const double* Fa, const int32_t* valida, const double* Fb, const int32_t* validb, int n, double* d,
                           mmh_stream_t s) {
    MMH_REQUIRE(Fa && valida && Fb && validb && d, "mmh_pose_pair_distance (pose_knn): NULL argument");
    MMH_REQUIRE(n >= 1, "mmh_pose_pair_distance (pose_knn): n = %d (at least 1 pair)", n);
    hipLaunchKernelGGL(pose_pair_distance_kernel, dim3((unsigned)mmh::cdiv(n, 256)), dim3(256), 0, mmh::as_stream(s), Fa, valida, Fb,
                       validb, n, d);
    return mmh::check_launch("pose_pair_distance");
}

// Top-k selection of the pose-distance search (pose_knn.hip), shared by host and device: a sorted list of K entries under one
// TOTAL order - larger cosine first, then smaller candidate index - so that the k best of a set do not depend on the order
// its elements arrive in, nor on how the set was cut into tiles, lane groups, waves or slices.  Every loop has a compile-time
// trip count and compile-time indices: on the device a list lives in registers.
//
// An empty slot is (cos = -infinity, idx = POSE_TOPK_EMPTY): it ranks after every real entry (cosines are finite, indices
// are below 2^31 - 1), so "fewer than K entries" needs no count.
//
// make pose_topk_host_check: pose_topk_host_check.cpp drives insert and merge against std::sort under ASan + UBSan.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define POSE_HD __host__ __device__ __forceinline__
#define POSE_UNROLL _Pragma("unroll")
#else
#define POSE_HD inline
#define POSE_UNROLL
#endif

constexpr int32_t POSE_TOPK_EMPTY = 0x7fffffff;
constexpr int POSE_TOPK_MAX = 16;

POSE_HD double pose_topk_neg_inf() { return -__builtin_huge_val(); }

// a ranks strictly before b
POSE_HD bool pose_before(double ca, int32_t ia, double cb, int32_t ib) { return ca > cb || (ca == cb && ia < ib); }

template <int K>
struct PoseTopK {
    double c[K];
    int32_t i[K];

    POSE_HD void clear() {
POSE_UNROLL
        for (int j = 0; j < K; ++j) {
            c[j] = pose_topk_neg_inf();
            i[j] = POSE_TOPK_EMPTY;
        }
    }

    // insert (cv, iv) if it ranks before the last entry; the list stays sorted.  An entry equal to one already held (same
    // cosine AND same index) is not before it and would be kept twice: callers feed every candidate once.
    POSE_HD void insert(double cv, int32_t iv) {
        if (!pose_before(cv, iv, c[K - 1], i[K - 1])) return;
POSE_UNROLL
        for (int j = K - 1; j >= 0; --j) {
            // slot j takes its left neighbour when the new entry ranks before that neighbour, the new entry when it ranks
            // before slot j only, and keeps its own otherwise (the entries on the right were moved by the earlier steps)
            const bool shift = j > 0 && pose_before(cv, iv, c[j > 0 ? j - 1 : 0], i[j > 0 ? j - 1 : 0]);
            const bool here = pose_before(cv, iv, c[j], i[j]);
            const double nc = shift ? c[j > 0 ? j - 1 : 0] : (here ? cv : c[j]);
            const int32_t ni = shift ? i[j > 0 ? j - 1 : 0] : (here ? iv : i[j]);
            c[j] = nc;
            i[j] = ni;
        }
    }

    // merge n entries of a sorted (or unsorted) list stored with a stride; empty slots are skipped by the order itself
    POSE_HD void merge(const double* oc, const int32_t* oi, int n, int stride) {
        for (int j = 0; j < n; ++j) {
            const int32_t iv = oi[j * stride];
            if (iv != POSE_TOPK_EMPTY) insert(oc[j * stride], iv);
        }
    }
};

// the list size compiled for a requested k (1 .. 16): the next of 1, 2, 4, 8, 16.  The first k entries of the best KT are the
// best k, because the order is total.
POSE_HD int pose_topk_size(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

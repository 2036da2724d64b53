// Compacted-channel fp32 kernels for the 7x7 / stride-1 / ReflectionPad2d(3) stems whose input is mostly pose heat maps
// (models/Generator.py:158-164 pose stem, models/Discriminator.py:60-64 D_PB): a truncated Gaussian covers about 1.6 % of a
// 256 x 256 map, so a 16 x 16 output tile with its halo sees a given pose channel with probability of about 5 % - the dense
// kernels (conv_stem_f32.hip, conv_stem.hip, conv_igemm.hip) multiply zeros for the rest.
//
//   stem_activity_kernel   one pass over x: per 8 x 16 pixel block (plus the 3-pixel halo, through the reflection index map)
//                          a 64-bit word whose bit c says "channel c has a non-zero element there".  Exact, not conservative.
//   stem_sparse_fprop      conv_stem_f32_kernel's output tile, wave-to-pixel mapping, accumulators and epilogue
//                          (stem_f32_epilogue.h) with the contraction running over the tile's ACTIVE channels only, in the
//                          dense kernel's order.  The fp32 MFMA is a k-ordered fmaf chain and an omitted term is
//                          fmaf(0, w, acc) = acc for finite w, so y and the statistics are the dense kernel's bit for bit
//                          (an accumulator that is exactly -0.0 stays -0.0 here and becomes +0.0 there: equal as floats).
//                          Non-finite WEIGHTS are outside the guarantee: 0 * inf is NaN in the dense kernel, skipped here.
//   stem_sparse_wgrad      channel-centric: a workgroup owns one input channel and one of the dense stem wgrad's splits, and
//                          runs a [49 taps -> 64] x [64] x [128 pixels] MFMA GEMM for every 2 x 64 pixel tile of the split
//                          in which the channel is active, in the dense kernel's order: dw is conv_stem.hip's bit for bit.
//                          Slabs [splits][7][7][C][64], summed by slab_reduce.hip exactly as the dense kernel's are.
//   stem_sparse_wgrad_flat the same for the stems whose dense route is the generic wgrad of conv_igemm.hip (D_PB, 24 lanes): a
//                          workgroup owns four adjacent channels and one of THAT kernel's splits of the flat pixel range and
//                          multiplies a 32-pixel k-step only for the channels that are active in it: dw is conv_igemm.hip's
//                          bit for bit.
//
// Plain global loads and LDS reads / writes only; no LDS-DMA, no cross-workgroup waits, no atomics; every loop is bounded by
// a count read once.  The results never depend on the sparsity: a tile with every channel active runs the same loops.
#include <algorithm>
#include "stem_f32_epilogue.h"

namespace mmh { int g_stem_sparse = 1, g_stem_sparse_flat = 1; }

namespace {
using namespace mmh::dev;

constexpr int BR = 8, BC = 16;                  // mask block: 8 x 16 output pixels
constexpr int HC = BC + 6;                      // halo width of a block / tile
constexpr int CMAX = 48;

__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// ---------------------------------------------------------------------------------------------------- activity mask
__global__ void __launch_bounds__(256) stem_activity_kernel(const float* __restrict__ x, unsigned long long* __restrict__ mask,
                                                            int H, int W, int C) {
    __shared__ unsigned long long part[4];
    const int bx = blockIdx.x, by = blockIdx.y, b = blockIdx.z;
    const int c4 = C >> 2;
    const int units = (BR + 6) * HC * c4;       // float4 reads of the block's 14 x 22 pixel window
    unsigned long long bits = 0;
    for (int u = threadIdx.x; u < units; u += 256) {
        const int px = u / c4, q = u - px * c4;
        const int hr = px / HC, hc = px - hr * HC;
        const int ih = reflect_idx(by * BR - 3 + hr, H), iw = reflect_idx(bx * BC - 3 + hc, W);
        const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)(b * H + ih) * W + iw) * (size_t)C + 4 * q);
        // -0.0 != 0 is false, NaN != 0 is true
        const unsigned nz = (v.x != 0.f ? 1u : 0u) | (v.y != 0.f ? 2u : 0u) | (v.z != 0.f ? 4u : 0u) | (v.w != 0.f ? 8u : 0u);
        bits |= (unsigned long long)nz << (4 * q);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)bits, s, 64), hi = __shfl_xor((unsigned)(bits >> 32), s, 64);
        bits |= ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0)
        mask[((size_t)b * gridDim.y + by) * gridDim.x + bx] = part[0] | part[1] | part[2] | part[3];
}

// ---------------------------------------------------------------------------------------------------- fprop
constexpr int FNT = 512;
// Two launches share the tiles by their number of active channels: tiles with at most CAP_LO of them run from a small LDS
// image (CAP_LO planes, a CH_LO-row filter stage: 52 KiB, and the MT = 2 kernel compiles to 77 VGPRs, no AGPRs - three
// workgroups of 8 waves fit a CU by both counts; not measured by counter), the others from one that holds every channel
// (one workgroup per CU).  A workgroup whose tile belongs to the other launch returns at once.  7 * 14 = 98: the whole
// filter of a two-channel tile in one stage.
constexpr int CAP_LO = 12, CH_LO = 98, CH_HI = 224;

struct SparseFpropKP {
    const float* x;         // [B][H][W][x_cs]
    const unsigned long long* mask;     // [B][H/8][W/16]
    const float* w;         // [7][7 Cin][64]
    const float* bias;
    float* y;               // [B][H][W][y_cs]
    float* stats;           // [tiles * 4][3][64] or null
    int B, H, W, Cin, x_cs, y_cs, J, TX, TY;
    int cap, ch;            // planes and filter rows (even) the LDS image holds
    int lo, hi;             // this launch takes the tiles with lo <= active channels <= hi
};

// LDS: wave counts [8] | entry list [7 Cin + 1] (plane byte offset + 4 kw, filter row j) | planes [cap + 1][HR][HC] | filter stage [ch][64]
template <int MT>
__global__ void __launch_bounds__(FNT, 1) stem_sparse_fprop_kernel(const SparseFpropKP p) {
    constexpr int TR = 8 * MT, HR = TR + 6, PLANE = HR * HC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, kg = lane >> 5;
    const int pg = wave & 3, nh = wave >> 2;
    int* wave_cnt = reinterpret_cast<int*>(smem);       // [8]
    int2* ent = reinterpret_cast<int2*>(smem + 32);
    const int ent_b = 32 + (((7 * p.Cin + 1) * 8 + 15) & ~15);
    float* planes = reinterpret_cast<float*>(smem + ent_b);
    float* wst = planes + (p.cap + 1) * PLANE;

    const int tile = blockIdx.x;
    const int tpi = p.TX * p.TY;
    const int b = tile / tpi;
    const int trem = tile - b * tpi;
    const int ty = trem / p.TX, tx = trem - ty * p.TX;

    // the tile's active channels: OR of its blocks' words
    unsigned long long act = 0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) act |= p.mask[((size_t)b * (p.H / BR) + ty * MT + mt) * (p.W / BC) + tx];
    const int nact = __popcll(act);
    if (nact < p.lo || nact > p.hi) return;             // the other launch's tile (uniform: before any barrier)
    const int Lr = 7 * nact, Lp = (Lr + 1) & ~1;
    const int CH = p.ch;

    // the list of one filter row: the dense kernel walks j = kw Cin + c in k-steps of 8, MFMA t of a step taking j = 8 g + t
    // (k slot 0) then 8 g + 4 + t (slot 1).  Position `tid` of that order keeps its rank among the active ones.
    {
        const int g = tid >> 3, r = tid & 7;
        const int j = 8 * g + 4 * (r & 1) + (r >> 1);
        const int kw = j / p.Cin, c = j - kw * p.Cin;
        const bool on = j < p.J && ((act >> c) & 1ull);
        const unsigned long long bal = __ballot(on);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int rank = __popcll(bal & ((1ull << lane) - 1ull));
        for (int v = 0; v < wave; ++v) rank += wave_cnt[v];
        if (on) ent[rank] = make_int2(__popcll(act & ((1ull << c) - 1ull)) * (PLANE * 4) + 4 * kw, j);
        if (tid == 0 && Lp > Lr) ent[Lr] = make_int2(nact * (PLANE * 4), 0);       // the plane of zeros, any finite filter row
    }
    // the active channels' halo planes (reflection folded into the source index) and the plane of zeros
    for (int u = tid; u < (nact + 1) * PLANE; u += FNT) {
        const int a = u / PLANE, px = u - a * PLANE;
        float v = 0.f;
        if (a < nact) {
            // channel of plane a: the a-th set bit of act
            unsigned long long t = act;
            for (int i = 0; i < a; ++i) t &= t - 1;
            const int c = __ffsll((long long)t) - 1;
            const int hr = px / HC, hc = px - hr * HC;
            const int ih = reflect_idx(ty * TR - 3 + hr, p.H), iw = reflect_idx(tx * BC - 3 + hc, p.W);
            v = p.x[((size_t)(b * p.H + ih) * p.W + iw) * (size_t)p.x_cs + c];
        }
        planes[u] = v;
    }

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

    // lane constants: pixel (tile row 2 pg + m / 16 (+ 8 mt), column m % 16), filter column 32 nh + m
    const int a_lane = ((2 * pg + (m >> 4)) * HC + (m & 15)) * 4;
    const int n = 32 * nh + m;
    const char* const planes_c = reinterpret_cast<const char*>(planes);

    // stages: whole filter rows while a row's list fits CH entries, else pieces of one row.  kh outermost, the list inside:
    // the dense kernel's order
    const int khg = Lp <= CH ? (Lp ? min(7, CH / Lp) : 7) : 1;
    const int cw = Lp <= CH ? Lp : CH;
    for (int kh0 = 0; kh0 < 7; kh0 += khg) {
        const int nk = min(khg, 7 - kh0);
        for (int c0 = 0; c0 < Lp; c0 += cw) {
            const int ne = min(cw, Lp - c0);        // even: cw and Lp are
            __syncthreads();                        // list and planes written / the previous stage read by every wave
            for (int u = tid; u < nk * ne * 16; u += FNT) {
                const int rr = u >> 4, q = u & 15;
                const int k = rr / ne, idx = rr - k * ne;
                const int j = ent[c0 + idx].y;
                *reinterpret_cast<float4*>(wst + rr * 64 + 4 * q) =
                    *reinterpret_cast<const float4*>(p.w + ((size_t)(kh0 + k) * p.J + j) * 64 + 4 * q);
            }
            __syncthreads();
            for (int k = 0; k < nk; ++k) {
                const int arow = a_lane + (kh0 + k) * (HC * 4);
                const float* wk = wst + k * ne * 64 + n;
                for (int i = 0; i < ne; i += 2) {
                    const int e = ent[c0 + i + kg].x;
                    const float bw = wk[(i + kg) * 64];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const float av = *reinterpret_cast<const float*>(planes_c + e + arow + mt * 8 * (HC * 4));
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bw, acc[mt], 0, 0, 0);
                    }
                }
            }
        }
    }
    const float bv = p.bias ? p.bias[n] : 0.f;
    stem_f32_epilogue<MT>(acc, p.y, p.stats, tile, b, ty, tx, pg, kg, n, bv, p.H, p.W, p.y_cs, MMH_ACT_NONE);
}

// the dense kernel's tile height for this conv, from the partials it writes: 4 rows of partials per 8 MT x 16 pixel tile
int dense_mt(const mmh_conv_desc* d) {
    if (d->H % BR || d->W % BC) return 0;
    const int chunks = mmh::stem_f32_stats_chunks(d);
    if (chunks <= 0) return 0;
    const int mt = d->B * (d->H / BR) * (d->W / BC) * 4 / chunks;
    return (mt == 1 || mt == 2) ? mt : 0;
}

size_t fprop_lds(int Cin, int mt, int cap, int ch) {
    return 32 + (size_t)(((7 * Cin + 1) * 8 + 15) & ~15) + (size_t)(cap + 1) * (8 * mt + 6) * HC * 4 + (size_t)ch * 256;
}

bool fprop_ok(const mmh_conv_desc* d) {
    if (!d || !mmh::stem_f32_ok(d) || d->pad_mode != MMH_PAD_REFLECT || d->Cin > CMAX) return false;
    if (mmh::g_stem_f32_levels != 1) return false;      // the dense kernel's phase boundaries cut through the compacted list
    const int mt = dense_mt(d);
    return mt && d->H >= 4 && d->W >= 4 && fprop_lds(d->Cin, mt, d->Cin, CH_HI) <= 160 * 1024;
}

// ---------------------------------------------------------------------------------------------------- wgrad
// The dense stem wgrad (conv_stem.hip, stem_wgrad_kernel) sums, per element of dw, ONE fmaf chain per split over the
// split's tiles of 2 x 64 pixels (columns fastest, then rows, then images) and, inside a tile, over its 128 pixels in
// row-major order, then adds the splits' slabs with slab_reduce.  This kernel keeps the tiles, the splits, the pixel
// order and the slab sum and leaves out the tiles in which the channel is all zero: fmaf(0, dy, acc) = acc for finite dy,
// so dw is the dense kernel's bit for bit (up to the sign of an exact zero).
constexpr int WNT = 256;
constexpr int WTR = 2, WTC = 64;                // the dense kernel's tile
constexpr int WP = WTR * WTC;                   // 128 pixels per tile
constexpr int WHC = WTC + 6, WHPL = (WTR + 6) * WHC;        // halo plane of a tile: 8 x 70 pixels
constexpr int WNH = (WHPL + WNT - 1) / WNT;     // halo loads per thread

struct SparseWgradKP {
    const float* x;         // [B][H][W][x_cs]
    const unsigned long long* mask;     // [B][H/8][W/16]
    const float* dy;        // [B][H][W][y_cs]
    float* slab;            // [splits][49][Cin][64]
    int H, W, Cin, x_cs, y_cs, BX, BY, tw, th, tiles, tiles_per_split;
};

// one tile's operands into registers: its dy [128][64] (8 float4 per thread) and channel c's 8 x 70 halo plane
__device__ __forceinline__ void wgrad_fetch(const SparseWgradKP& p, int t, int c, int tid, float4 (&dreg)[8], float (&hreg)[WNH]) {
    const int wx = t % p.tw, hy = (t / p.tw) % p.th, b = t / (p.tw * p.th);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = u * WNT + tid;            // float4 e of the tile's [128][64]
        const int px = e >> 4, q = e & 15;
        const int oh = hy * WTR + (px >> 6), ow = wx * WTC + (px & 63);
        dreg[u] = *reinterpret_cast<const float4*>(p.dy + ((size_t)(b * p.H + oh) * p.W + ow) * (size_t)p.y_cs + 4 * q);
    }
#pragma unroll
    for (int u = 0; u < WNH; ++u) {
        const int e = min(u * WNT + tid, WHPL - 1);         // the last threads repeat the last pixel and do not store it
        const int hr = e / WHC, hc = e - hr * WHC;
        const int ih = reflect_idx(hy * WTR - 3 + hr, p.H), iw = reflect_idx(wx * WTC - 3 + hc, p.W);
        hreg[u] = p.x[((size_t)(b * p.H + ih) * p.W + iw) * (size_t)p.x_cs + c];
    }
}

// workgroup (c, split): 4 waves = (tap half mh, output-channel half nh), one 32x32 accumulator each: rows = taps 32 mh + .,
// columns = output channels 32 nh + .; per active tile 64 MFMA 32x32x2 over its 128 pixels.
// LDS: dy of the tile [128][64] | halo plane [8][70] | list of the split's active tiles [tiles_per_split]
__global__ void __launch_bounds__(WNT) stem_sparse_wgrad_kernel(const SparseWgradKP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int wave_cnt[4];
    float* dys = reinterpret_cast<float*>(smem);
    float* halo = dys + WP * 64;
    int* list = reinterpret_cast<int*>(halo + WHPL);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, kg = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    const int c = blockIdx.x, split = blockIdx.y;
    const int t0 = split * p.tiles_per_split;
    const int nt = max(0, min(p.tiles_per_split, p.tiles - t0));

    // the split's tiles that have channel c, ascending: a tile lies in one row of mask blocks and covers four of them, and
    // its 3-pixel halo lies inside theirs
    int nlist = 0;
    for (int i0 = 0; i0 < nt; i0 += WNT) {
        const int i = i0 + tid;
        bool on = false;
        if (i < nt) {
            const int t = t0 + i;
            const int wx = t % p.tw, hy = (t / p.tw) % p.th, b = t / (p.tw * p.th);
            const unsigned long long* mw = p.mask + ((size_t)b * p.BY + (hy * WTR) / BR) * p.BX + wx * (WTC / BC);
            on = (((mw[0] | mw[1] | mw[2] | mw[3]) >> c) & 1ull) != 0;
        }
        const unsigned long long bal = __ballot(on);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int rank = nlist + __popcll(bal & ((1ull << lane) - 1ull));
        for (int v = 0; v < wave; ++v) rank += wave_cnt[v];
        if (on) list[rank] = t0 + i;
        nlist += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    // this lane's tap (rows past 48 repeat tap 48 and are not stored) as a halo offset
    const int tap = min(32 * mh + m, 48);
    const int a_lane = (tap / 7) * WHC + (tap % 7);

    float4 dreg[8];
    float hreg[WNH];
#pragma unroll
    for (int u = 0; u < 8; ++u) dreg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < WNH; ++u) hreg[u] = 0.f;
    if (nlist > 0) wgrad_fetch(p, list[0], c, tid, dreg, hreg);
    for (int a = 0; a < nlist; ++a) {
#pragma unroll
        for (int u = 0; u < 8; ++u) *reinterpret_cast<float4*>(dys + (u * WNT + tid) * 4) = dreg[u];
#pragma unroll
        for (int u = 0; u < WNH; ++u)
            if (u * WNT + tid < WHPL) halo[u * WNT + tid] = hreg[u];
        __syncthreads();
        if (a + 1 < nlist) wgrad_fetch(p, list[a + 1], c, tid, dreg, hreg);
        const float* bcol = dys + 32 * nh + m;
        // MFMA i: pixel 2 i in k slot 0, 2 i + 1 in slot 1 - the dense kernel's pairs
#pragma unroll 8
        for (int i = 0; i < WP / 2; ++i) {
            const int px = 2 * i + kg;
            const float av = halo[a_lane + (px >> 6) * WHC + (px & 63)];
            const float bw = bcol[px * 64];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bw, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* out = p.slab + (size_t)split * 49 * p.Cin * 64 + (size_t)c * 64 + 32 * nh + m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = 32 * mh + (r & 3) + 8 * (r >> 2) + 4 * kg;
        if (t < 49) out[(size_t)t * p.Cin * 64] = acc[r];
    }
}

bool wgrad_ok(const mmh_conv_desc* d) {
    return d && d->kh == 7 && d->kw == 7 && d->stride == 1 && d->pad == 3 && d->pad_mode == MMH_PAD_REFLECT &&
           d->dtype == MMH_F32 && d->Cout == 64 && d->y_cs >= 64 && d->y_cs % 4 == 0 && d->Cin >= 4 && d->Cin <= CMAX &&
           d->Cin % 4 == 0 && d->x_cs >= d->Cin && d->H % BR == 0 && d->W % WTC == 0 && d->H >= 4 && d->W >= 4 &&
           d->Ho == d->H && d->Wo == d->W && d->B >= 1 &&
           (size_t)d->B * d->H * d->W * std::max(d->x_cs, d->y_cs) < (1ull << 31);
}

// the dense kernel's split rule (conv_stem.hip: stem_khg, stem_splits): 512 workgroups over its groups of filter rows.
// tests/test_stem_sparse_cpu.py holds the two workspace sizes against each other.
void wgrad_splits(const mmh_conv_desc* d, int& tiles, int& tiles_per_split, int& splits) {
    tiles = d->B * (d->H / WTR) * (d->W / WTC);
    int khg = (14 * 32) / (7 * d->Cin);
    khg = khg < 1 ? 1 : (khg > 7 ? 7 : khg);
    const int groups = (7 + khg - 1) / khg;
    splits = std::max(1, 512 / groups);
    splits = std::min(splits, tiles);
    tiles_per_split = (tiles + splits - 1) / splits;
}

// ---------------------------------------------------------------------------------------------------- wgrad, flat order
// The generic wgrad (conv_igemm.hip, conv_wgrad_kernel + slab_reduce) is the dense route of the stems conv_stem.hip does
// not take (D_PB: 24 lanes).  Per element of dw it sums ONE fmaf chain per split over the split's flat range of dy-domain
// pixels (image, row, column ascending) in k-steps of 32 pixels, pixel 2 i of a step in k slot 0 of MFMA i and 2 i + 1 in
// slot 1.  This kernel keeps the splits (mmh::wgrad_flat_split), the steps, the pairs and the slab sum, and leaves out the
// steps in which a lane is all zero: dw is the generic kernel's bit for bit (up to the sign of an exact zero, finite dy).
//
// A workgroup owns a group of four adjacent lanes (one float4 of x per pixel) and a split.  W % 16 == 0 and 32-aligned steps
// put each 16-pixel half of a step inside one 8 x 16 mask block - the second half on the next row where the step crosses a
// row end - whose word covers the halo of every tap; a step is multiplied for the lanes whose bit either half has.
// Lanes that are active everywhere (D_PB's three image lanes, wherever they sit) so share one pass over dy with their
// group instead of taking one each, and a group of four sparse lanes reads dy only where one of them is active.
constexpr int FS = 32;                          // pixels per step: the generic kernel's k-step
constexpr int FHP = 7 * HC;                     // halo of a 16-pixel half: 7 rows x 22 columns
constexpr int FNH = 2 * FHP;                    // halo pixels of a step
constexpr int FCH = 256;                        // steps listed at a time, one per thread

struct FlatWgradKP {
    const float* x;         // [B][H][W][x_cs]
    const unsigned long long* mask;     // [B][H/8][W/16]
    const float* dy;        // [B][H][W][y_cs]
    float* slab;            // [splits][49][Cin][64]
    int H, W, Cin, x_cs, y_cs, BX, BY, P, pix_per_split;
};

// one step's operands into registers: its dy [32][64] (2 float4 per thread) and the lane group's halo (308 float4)
__device__ __forceinline__ void flat_fetch(const FlatWgradKP& p, int step, int g, int tid, float4 (&dreg)[2], float4 (&hreg)[2]) {
    const int pix0 = step * FS, HW = p.H * p.W;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = u * 256 + tid;            // float4 e of the step's [32][64]
        dreg[u] = *reinterpret_cast<const float4*>(p.dy + (size_t)(pix0 + (e >> 4)) * (size_t)p.y_cs + 4 * (e & 15));
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = min(u * 256 + tid, FNH - 1);          // the last threads repeat the last pixel and do not store it
        const int half = e / FHP, r = e - half * FHP;
        const int hr = r / HC, hc = r - hr * HC;
        const int pix = pix0 + 16 * half;
        const int b = pix / HW, rem = pix - b * HW;
        const int row = rem / p.W, col = rem - row * p.W;
        const int ih = reflect_idx(row - 3 + hr, p.H), iw = reflect_idx(col - 3 + hc, p.W);
        hreg[u] = *reinterpret_cast<const float4*>(p.x + ((size_t)(b * p.H + ih) * p.W + iw) * (size_t)p.x_cs + 4 * g);
    }
}

// workgroup (lane group g, split): 4 waves = (tap half mh, output-channel half nh), one 32x32 accumulator per lane of the
// group: rows = taps 32 mh + ., columns = output channels 32 nh + .; per active step and active lane 16 MFMA 32x32x2.
__global__ void __launch_bounds__(256) stem_sparse_wgrad_flat_kernel(const FlatWgradKP p) {
    __shared__ __attribute__((aligned(16))) float dys[FS * 64];
    __shared__ float planes[4 * FNH];           // [lane of the group][half][7][22]
    __shared__ int list[FCH];                   // active steps of the chunk, ascending: step | lanes << 24 (step < 2^20)
    __shared__ int wave_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, kg = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    // splits along x: the workgroups of one group - of the always-active lanes' above all - are consecutive in dispatch order
    // and so spread evenly over the XCDs and CUs (group along x would put them on every other XCD: 24 lanes = 6 groups).
    // Groups in the order first, last, second, ...: image lanes in front of the pose maps or behind them both start at once
    // (scheduling only: every group runs the same code; in plain order image lanes at 21-23 come last and stack on the CUs
    // that free up first: 2969 us against 1625 at B = 64, 256 x 256)
    const int gy = blockIdx.y, split = blockIdx.x;
    const int g = (gy & 1) ? (int)gridDim.y - 1 - (gy >> 1) : (gy >> 1);
    const int HW = p.H * p.W;
    const int pbeg = split * p.pix_per_split;
    const int pend = min(p.P, pbeg + p.pix_per_split);
    const int s0 = pbeg / FS;
    const int ns = pend > pbeg ? (pend - pbeg) / FS : 0;        // P % 32 == 0: whole steps only; a split past P is empty

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
    // this lane's tap (rows past 48 repeat tap 48 and are not stored) as a halo offset
    const int tap = min(32 * mh + m, 48);
    const int a_lane = (tap / 7) * HC + (tap % 7);

    float4 dreg[2], hreg[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) dreg[u] = hreg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c0 = 0; c0 < ns; c0 += FCH) {
        // the chunk's steps in which a lane of the group is active
        int lanes = 0;
        if (c0 + tid < ns) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pix = (s0 + c0 + tid) * FS + 16 * h;
                const int b = pix / HW, rem = pix - b * HW;
                const int row = rem / p.W, col = rem - row * p.W;
                lanes |= (int)((p.mask[((size_t)b * p.BY + row / BR) * p.BX + col / BC] >> (4 * g)) & 15ull);
            }
        }
        const bool on = lanes != 0;
        const unsigned long long bal = __ballot(on);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int rank = __popcll(bal & ((1ull << lane) - 1ull));
        for (int v = 0; v < wave; ++v) rank += wave_cnt[v];
        if (on) list[rank] = (s0 + c0 + tid) | (lanes << 24);
        const int nlist = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();

        if (nlist > 0) flat_fetch(p, list[0] & 0xffffff, g, tid, dreg, hreg);
        for (int a = 0; a < nlist; ++a) {
            const int act = __builtin_amdgcn_readfirstlane(list[a]) >> 24;
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<float4*>(dys + (u * 256 + tid) * 4) = dreg[u];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = u * 256 + tid;
                if (e < FNH) {
                    planes[e] = hreg[u].x; planes[FNH + e] = hreg[u].y;
                    planes[2 * FNH + e] = hreg[u].z; planes[3 * FNH + e] = hreg[u].w;
                }
            }
            __syncthreads();
            if (a + 1 < nlist) flat_fetch(p, list[a + 1] & 0xffffff, g, tid, dreg, hreg);
            // MFMA i: pixel 2 i in k slot 0, 2 i + 1 in slot 1 - the generic kernel's pairs
            float bw[FS / 2];
#pragma unroll
            for (int i = 0; i < FS / 2; ++i) bw[i] = dys[(2 * i + kg) * 64 + 32 * nh + m];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if ((act >> q) & 1) {
                    float av[FS / 2];           // all 16 reads first, then the MFMAs back to back
#pragma unroll
                    for (int i = 0; i < FS / 2; ++i) {
                        const int px = 2 * i + kg;
                        av[i] = planes[q * FNH + (px >> 4) * FHP + a_lane + (px & 15)];
                    }
                    asm volatile("" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]), "+v"(av[4]), "+v"(av[5]), "+v"(av[6]),
                                 "+v"(av[7]), "+v"(av[8]), "+v"(av[9]), "+v"(av[10]), "+v"(av[11]), "+v"(av[12]), "+v"(av[13]),
                                 "+v"(av[14]), "+v"(av[15]));     // keeps the scheduler from sinking each read to its MFMA
#pragma unroll
                    for (int i = 0; i < FS / 2; ++i) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bw[i], acc[q], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }
    // every row of the group in this split's slab, also where nothing fired (the workspace is not zeroed).
    // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* out = p.slab + (size_t)split * 49 * p.Cin * 64 + (size_t)(4 * g) * 64 + 32 * nh + m;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = 32 * mh + (r & 3) + 8 * (r >> 2) + 4 * kg;
            if (t < 49) out[((size_t)t * p.Cin + q) * 64] = acc[q][r];
        }
}

bool wgrad_flat_ok(const mmh_conv_desc* d) {
    return d && d->kh == 7 && d->kw == 7 && d->stride == 1 && d->pad == 3 && d->pad_mode == MMH_PAD_REFLECT &&
           d->dtype == MMH_F32 && d->Cout == 64 && d->y_cs >= 64 && d->y_cs % 4 == 0 && d->Cin >= 4 && d->Cin <= CMAX &&
           d->Cin % 4 == 0 && d->x_cs >= d->Cin && d->x_cs % 4 == 0 && d->H >= 8 && d->W >= 16 && d->H % BR == 0 &&
           d->W % BC == 0 && d->Ho == d->H && d->Wo == d->W && d->B >= 1 &&
           (size_t)d->B * d->H * d->W < (1ull << 31) / 64;
}

bool mask_args_ok(int B, int H, int W) {
    return B >= 1 && H >= 4 && W >= 4 && H % BR == 0 && W % BC == 0;
}

}  // namespace

extern "C" {

size_t mmh_stem_activity_bytes(int B, int H, int W) {
    return mask_args_ok(B, H, W) ? (size_t)B * (H / BR) * (W / BC) * 8 : 0;
}

int mmh_stem_activity(const void* x, int B, int H, int W, int C, void* mask, mmh_stream_t s) {
    MMH_REQUIRE(mask_args_ok(B, H, W), "mmh_stem_activity: needs H %% 8 == 0, W %% 16 == 0, H, W >= 4 (got %d x %d x %d)", B, H, W);
    MMH_REQUIRE(C >= 4 && C <= CMAX && C % 4 == 0, "mmh_stem_activity: needs 4 <= C <= 48, C %% 4 == 0 (got %d)", C);
    MMH_REQUIRE((size_t)B * H * W * C < (1ull << 31), "mmh_stem_activity: tensor too large");
    MMH_REQUIRE(x && mask, "mmh_stem_activity: NULL buffer");
    MMH_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)mask & 7) == 0, "mmh_stem_activity: x needs 16-byte, mask 8-byte alignment");
    MMH_REQUIRE(H / BR <= 65535 && B <= 65535, "mmh_stem_activity: grid too large");
    hipLaunchKernelGGL(stem_activity_kernel, dim3(W / BC, H / BR, B), dim3(256), 0, mmh::as_stream(s),
                       static_cast<const float*>(x), static_cast<unsigned long long*>(mask), H, W, C);
    return mmh::check_launch("stem_activity_kernel");
}

int mmh_conv7_stem_sparse_fprop_supported(const mmh_conv_desc* d) { return mmh::g_stem_sparse && fprop_ok(d) ? 1 : 0; }

int mmh_conv7_stem_sparse_fprop(const mmh_conv_desc* d, const void* x, const void* mask, const void* w, const void* bias,
                                void* y, void* stats, mmh_stream_t s) {
    MMH_REQUIRE(fprop_ok(d), "mmh_conv7_stem_sparse_fprop: needs an fp32 7x7 / stride 1 / reflect pad 3 stem, Cin %% 4 == 0 "
                             "<= 48, Cout == 64, whole dense-kernel tiles, conv_levels 1");
    MMH_REQUIRE(x && mask && w && y, "mmh_conv7_stem_sparse_fprop: NULL buffer");
    MMH_REQUIRE(((uintptr_t)w & 15) == 0 && ((uintptr_t)mask & 7) == 0 && ((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0,
                "mmh_conv7_stem_sparse_fprop: w needs 16-byte, mask 8-byte alignment");
    const int mt = dense_mt(d);
    SparseFpropKP p{};
    p.x = static_cast<const float*>(x);
    p.mask = static_cast<const unsigned long long*>(mask);
    p.w = static_cast<const float*>(w);
    p.bias = static_cast<const float*>(bias);
    p.y = static_cast<float*>(y);
    p.stats = static_cast<float*>(stats);
    p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.x_cs = d->x_cs; p.y_cs = d->y_cs; p.J = 7 * d->Cin;
    p.TX = d->W / BC; p.TY = d->H / (BR * mt);
    static int ready = -1;
    if (ready != 0) {
        for (const void* k : {reinterpret_cast<const void*>(stem_sparse_fprop_kernel<1>), reinterpret_cast<const void*>(stem_sparse_fprop_kernel<2>)}) {
            hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return mmh::fail("mmh_conv7_stem_sparse_fprop: %s", hipGetErrorString(e));
        }
        ready = 0;
    }
    const int tiles = p.B * p.TX * p.TY;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) { p.cap = std::min(CAP_LO, d->Cin); p.ch = CH_LO; p.lo = 0; p.hi = p.cap; }
        else { p.cap = d->Cin; p.ch = CH_HI; p.lo = CAP_LO + 1; p.hi = d->Cin; }
        if (p.lo > p.hi) break;
        const size_t lds = fprop_lds(d->Cin, mt, p.cap, p.ch);
        if (mt == 2) hipLaunchKernelGGL(stem_sparse_fprop_kernel<2>, dim3(tiles), dim3(FNT), lds, mmh::as_stream(s), p);
        else hipLaunchKernelGGL(stem_sparse_fprop_kernel<1>, dim3(tiles), dim3(FNT), lds, mmh::as_stream(s), p);
        if (int rc = mmh::check_launch("stem_sparse_fprop_kernel")) return rc;
    }
    return 0;
}

int mmh_conv7_stem_sparse_wgrad_supported(const mmh_conv_desc* d) { return mmh::g_stem_sparse && wgrad_ok(d) ? 1 : 0; }

size_t mmh_conv7_stem_sparse_wgrad_ws_bytes(const mmh_conv_desc* d) {
    if (!wgrad_ok(d)) return 0;
    int tiles, per, splits;
    wgrad_splits(d, tiles, per, splits);
    return (size_t)splits * 49 * d->Cin * 64 * sizeof(float);
}

int mmh_conv7_stem_sparse_wgrad(const mmh_conv_desc* d, const void* x, const void* mask, const void* dy, void* dw, void* ws,
                                size_t ws_bytes, int accumulate, mmh_stream_t s) {
    MMH_REQUIRE(wgrad_ok(d), "mmh_conv7_stem_sparse_wgrad: needs an fp32 7x7 / stride 1 / reflect pad 3 stem, Cin %% 4 == 0 <= 48, "
                             "Cout == 64, H %% 8 == 0, W %% 64 == 0");
    MMH_REQUIRE(x && mask && dy && dw && ws && ws_bytes >= mmh_conv7_stem_sparse_wgrad_ws_bytes(d),
                "mmh_conv7_stem_sparse_wgrad: bad buffers");
    MMH_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)dw & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)mask & 7) == 0 &&
                    ((uintptr_t)x & 3) == 0,
                "mmh_conv7_stem_sparse_wgrad: dy, dw, ws need 16-byte, mask 8-byte alignment");
    SparseWgradKP p{};
    p.x = static_cast<const float*>(x);
    p.mask = static_cast<const unsigned long long*>(mask);
    p.dy = static_cast<const float*>(dy);
    p.slab = static_cast<float*>(ws);
    p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.x_cs = d->x_cs; p.y_cs = d->y_cs;
    p.BX = d->W / BC; p.BY = d->H / BR; p.tw = d->W / WTC; p.th = d->H / WTR;
    int splits;
    wgrad_splits(d, p.tiles, p.tiles_per_split, splits);
    const size_t lds = (size_t)(WP * 64 + WHPL + p.tiles_per_split) * sizeof(float);
    MMH_REQUIRE(lds <= 64 * 1024, "mmh_conv7_stem_sparse_wgrad: tile list does not fit LDS");
    hipStream_t st = mmh::as_stream(s);
    hipLaunchKernelGGL(stem_sparse_wgrad_kernel, dim3(d->Cin, splits), dim3(WNT), lds, st, p);
    if (int rc = mmh::check_launch("stem_sparse_wgrad_kernel")) return rc;
    const int n4 = 49 * d->Cin * 64 / 4;
    return mmh::launch_slab_reduce(p.slab, static_cast<float*>(dw), n4, splits, accumulate, n4, st);
}

int mmh_conv7_stem_sparse_wgrad_flat_supported(const mmh_conv_desc* d) {
    return mmh::g_stem_sparse && mmh::g_stem_sparse_flat && wgrad_flat_ok(d) ? 1 : 0;
}

size_t mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(const mmh_conv_desc* d) {
    if (!wgrad_flat_ok(d)) return 0;
    int splits, pps;
    mmh::wgrad_flat_split(49 * d->Cin, 64, d->B * d->H * d->W, splits, pps);
    return (size_t)splits * 49 * d->Cin * 64 * sizeof(float);
}

int mmh_conv7_stem_sparse_wgrad_flat(const mmh_conv_desc* d, const void* x, const void* mask, const void* dy, void* dw, void* ws,
                                     size_t ws_bytes, int accumulate, mmh_stream_t s) {
    MMH_REQUIRE(wgrad_flat_ok(d), "mmh_conv7_stem_sparse_wgrad_flat: needs an fp32 7x7 / stride 1 / reflect pad 3 stem, Cin %% 4 == 0 "
                                  "<= 48, Cout == 64, H %% 8 == 0, W %% 16 == 0, B H W < 2^25");
    MMH_REQUIRE(x && mask && dy && dw && ws && ws_bytes >= mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(d),
                "mmh_conv7_stem_sparse_wgrad_flat: bad buffers");
    MMH_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)dw & 15) == 0 && ((uintptr_t)ws & 15) == 0 &&
                    ((uintptr_t)mask & 7) == 0,
                "mmh_conv7_stem_sparse_wgrad_flat: x, dy, dw, ws need 16-byte, mask 8-byte alignment");
    FlatWgradKP p{};
    p.x = static_cast<const float*>(x);
    p.mask = static_cast<const unsigned long long*>(mask);
    p.dy = static_cast<const float*>(dy);
    p.slab = static_cast<float*>(ws);
    p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.x_cs = d->x_cs; p.y_cs = d->y_cs;
    p.BX = d->W / BC; p.BY = d->H / BR; p.P = d->B * d->H * d->W;
    int splits;
    mmh::wgrad_flat_split(49 * d->Cin, 64, p.P, splits, p.pix_per_split);
    hipStream_t st = mmh::as_stream(s);
    hipLaunchKernelGGL(stem_sparse_wgrad_flat_kernel, dim3(splits, d->Cin / 4), dim3(256), 0, st, p);
    if (int rc = mmh::check_launch("stem_sparse_wgrad_flat_kernel")) return rc;
    const int n4 = 49 * d->Cin * 64 / 4;
    return mmh::launch_slab_reduce(p.slab, static_cast<float*>(dw), n4, splits, accumulate, n4, st);
}

}  // extern "C"

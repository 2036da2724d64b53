// Device-side primitives shared by the kernels of libmmhand_hip.so (gfx950 only): vector and LDS pointer types, the 16-bit
// MFMA wrappers, LDS fragment reads, LDS-DMA, the activation epilogue, the XCD work-item remap, the lane-pair store and the
// wave-level norm statistics.  One definition of each; a kernel file pulls them in with `using namespace mmh::dev;` inside
// its anonymous namespace.  Everything here is __forceinline__: one copy per translation unit.
#pragma once
#include "common.h"

namespace mmh { namespace dev {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_vp;
typedef const bf16x8 __attribute__((address_space(3))) * lds_frag_p;
typedef const float __attribute__((address_space(3))) * lds_f_p;
typedef const f32x4 __attribute__((address_space(3))) * lds_f4_p;

// The 16-bit MFMAs, named by instruction shape.  Operands are carried as 16-bit lanes typed bf16x8; H16 selects the fp16 opcode.
template <bool H16>
__device__ __forceinline__ f32x4 mfma_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
    if (H16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool H16>
__device__ __forceinline__ f32x16 mfma_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
    if (H16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// LDS reads at a 32-bit LDS byte address (lds_addr_of): one 16-bit MFMA fragment (ds_read_b128), one float, four floats;
// `imm` is a compile-time-constant byte offset that lands in the instruction's offset field
__device__ __forceinline__ bf16x8 lds_frag(unsigned addr) { return *reinterpret_cast<lds_frag_p>((size_t)addr); }
__device__ __forceinline__ float lds_f(unsigned addr, int imm = 0) { return *reinterpret_cast<lds_f_p>((size_t)(addr + (unsigned)imm)); }
__device__ __forceinline__ f32x4 lds_f4(unsigned addr, int imm = 0) { return *reinterpret_cast<lds_f4_p>((size_t)(addr + (unsigned)imm)); }

// One LDS-DMA instruction (global_load_lds_dwordx4: 1 KiB per wave, lane i -> lds_base + 16 i) as inline asm.
// Why not __builtin_amdgcn_global_load_lds: hipcc (ROCm 7.2) tracks the builtin as a pending LDS store and emits
// `s_waitcnt vmcnt(0)` in front of the next ds_read_b64_tr_b16 it cannot prove disjoint - right behind every issue,
// which drains a multi-stage ring once per step (seen in the ISA of the wgrad kernels; plain ds_read_b128 reads are not
// affected).  The asm form is invisible to that pass: the kernel orders DMA against reads itself (counted vmcnt +
// barrier).  M0 carries the LDS base (must be wave-uniform); kernels that use this must not use M0 otherwise.
__device__ __forceinline__ void lds_dma16(const void* g, unsigned lds_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_base) : "memory", "m0");
}
// LDS-DMA with a scalar base and a 32-bit lane offset (lds_dma16 takes a 64-bit pointer per lane)
__device__ __forceinline__ void dma16_s(const void* sbase, unsigned voff, unsigned lds_base) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_base) : "memory", "m0");
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}

// The epilogue activation of the MMH_ACT_* codes.  ReLU lets a NaN through, as torch.relu does (written `v > 0 ? v : 0` it
// compiled to v_max_f32, which answers 0 for a NaN: an overflow upstream came out of a fused conv + ReLU as a clean zero)
__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == MMH_ACT_RELU) return v <= 0.f ? 0.f : v;
    if (act == MMH_ACT_TANH) return tanhf(v);
    return v;
}

// Four consecutive output channels of one pixel from one lane (the accumulator layout of an MFMA 16x16x32 whose FIRST
// operand is the weight fragment: row = channel 4 g4 + r, column = pixel l15): bias, activation, one 8- or 16-byte store.
template <bool H16>
__device__ __forceinline__ void store4(float* y, char* y16, size_t elem, f32x4 v, const float* bv, int act) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act_apply(v[r] + bv[r], act);
    if (y16) {
        if (H16) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            h4 o = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            *reinterpret_cast<h4*>(y16 + elem * 2) = o;
        } else {
            typedef __bf16 b4 __attribute__((ext_vector_type(4)));
            b4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
            *reinterpret_cast<b4*>(y16 + elem * 2) = o;
        }
    } else {
        *reinterpret_cast<f32x4*>(y + elem) = v;
    }
}

// One XCD walks a contiguous range of work items (neighbours share data in its L2): launched with 8 * ceil(n / 8)
// workgroups, workgroup blockIdx.x (XCD blockIdx.x & 7) takes item xcd * ceil(n / 8) + blockIdx.x / 8.  Returns n for a
// workgroup past the end: `if (item >= n) return;`
__device__ __forceinline__ int xcd_item(int n) {
    const int per_xcd = (n + 7) / 8;
    const int item = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    return item < n ? item : n;
}

// One element of the norm backward, dx = k0*(dz - k1) - (x - mu)*k2 with dz = keep ? g/(1-p) : 0, as a
// PINNED sequence of operations (the empty asm statements stop the compiler from contracting it with
// its neighbours): norm_bwd_apply_v2 (pointwise.hip) and the backward transform that computes dx on
// the fly (wino6.hip) must round identically.
__device__ __forceinline__ float norm_bwd_elem(float g, bool keep, float dsc, float xv, float mu, float k0, float k1,
                                               float k2) {
    float dz = keep ? g * dsc : 0.f;
    asm volatile("" : "+v"(dz));
    float a = dz - k1;
    asm volatile("" : "+v"(a));
    float t = (xv - mu) * k2;
    asm volatile("" : "+v"(t));
    float o = __builtin_fmaf(k0, a, -t);
    asm volatile("" : "+v"(o));
    return o;
}

// Epilogue of the MFMA 16x16x32 kernels whose first operand is the weight fragment, 16-bit output: lane (l15 = pixel, g4) holds
// channels 4 g4 .. + 3 of each 16-channel column tile.  The lanes g4 and g4 ^ 1 (16 apart) trade one accumulator of a column
// tile PAIR (v_permlane16_swap: one instruction per register) - afterwards a lane holds EIGHT consecutive channels of its
// pixel, tile `even` from the even lane's side, tile `odd` from the odd lane's - and stores 16 bytes: half the store
// instructions, 64 contiguous bytes per pixel and instruction instead of 32 (the store shapes alone: 3.7 against 5.5 TB/s,
// tools/probes/store_pattern.hip).  v[0..7] on return: the lane's 8 channels, first channel = (g4 odd ? 16 : 0) + 4 (g4 & 2)
// of the 32-channel pair.  Every lane of the wave must call this (the swap is a cross-lane operation).
// (Inline asm: through __builtin_amdgcn_permlane16_swap hipcc 7.2 loses the instruction's second output in unrolled code.)
__device__ __forceinline__ void pair_swap8(const f32x4& even, const f32x4& odd, float* v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float lo = even[r], hi = odd[r];
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo), "+v"(hi));
        v[r] = lo;
        v[4 + r] = hi;
    }
}
template <bool H16>
__device__ __forceinline__ void store8_lp16(char* dst, const float* v) {
    if (H16) {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (_Float16)v[e];
        *reinterpret_cast<h8*>(dst) = o;
    } else {
        typedef __bf16 b8 __attribute__((ext_vector_type(8)));
        b8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
        *reinterpret_cast<b8*>(dst) = o;
    }
}

// Partial InstanceNorm statistics of a conv output tile from the epilogue of an MFMA 16x16x32 kernel whose FIRST operand is the
// weight fragment (lane (l15 = pixel, g4): channels 4 g4 + r, r < 4, of each of its NJ 16-channel column tiles, NV pixel
// rows per lane): count / mean / M2 of the wave's 16 NV pixels per channel, in the partial layout mmh_norm_stats_merge
// [_finalize] reduces ([.][3][N]: n, mean, M2).  val(i, j, r) = the value AS STORED (bias added, rounded to 16 bits) of row i,
// column tile j, register r.  Per lane two passes over its NV values per channel slot (4 j + r), then four equal-count Chan
// merges across the 16 pixel lanes as a reduce-scatter (ds_swizzle, xor 8 / 4 / 2 / 1): while a lane still holds more than
// one slot it keeps the half whose index bit matches its lane bit and hands the other half over; with one slot left the two
// partners merge and both keep the result (the lane whose remaining low bits are 0 writes).  sp: the partial's `n` row at
// this wave's first channel + 4 g4.  conv_lp16h2_kernel carries the NV = 8, NJ = 4 instance of the same scheme inline.
#define MMH_SWZ_(val, s) __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, val), 0x1f | ((s) << 10)))
template <int NS, int S>
__device__ __forceinline__ void wave_stats_step(float* m, float* q, int& ns, bool bit, float w) {
    if (ns > 1) {
        const int h = ns / 2;
#pragma unroll
        for (int c = 0; c < NS / 2; ++c) {
            if (c < h) {
                const float km = bit ? m[h + c] : m[c], sm = bit ? m[c] : m[h + c];
                const float kq = bit ? q[h + c] : q[c], sq = bit ? q[c] : q[h + c];
                const float om = MMH_SWZ_(sm, S), oq = MMH_SWZ_(sq, S), dl = om - km;
                q[c] = kq + oq + dl * dl * w;
                m[c] = 0.5f * (km + om);
            }
        }
        ns = h;
    } else {
        const float om = MMH_SWZ_(m[0], S), oq = MMH_SWZ_(q[0], S), dl = om - m[0];
        q[0] = q[0] + oq + dl * dl * w;
        m[0] = 0.5f * (m[0] + om);
    }
}
template <int NV, int NJ, typename F>
__device__ __forceinline__ void wave_tile_stats(F val, int l15, float* sp, int N) {
    constexpr int NS = 4 * NJ;
    float m[NS], q[NS];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v[NV], mean = 0.f, qq = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) { v[i] = val(i, j, r); mean += v[i]; }
            mean *= 1.f / NV;
#pragma unroll
            for (int i = 0; i < NV; ++i) qq = __builtin_fmaf(v[i] - mean, v[i] - mean, qq);
            m[4 * j + r] = mean; q[4 * j + r] = qq;
        }
    int ns = NS;
    wave_stats_step<NS, 8>(m, q, ns, (l15 & 8) != 0, 0.5f * NV);
    wave_stats_step<NS, 4>(m, q, ns, (l15 & 4) != 0, 1.0f * NV);
    wave_stats_step<NS, 2>(m, q, ns, (l15 & 2) != 0, 2.0f * NV);
    wave_stats_step<NS, 1>(m, q, ns, (l15 & 1) != 0, 4.0f * NV);
    // the slot this lane ends with: its lane bits, high to low, over the steps that still split (log2 NS of them)
    constexpr int SPLITS = NS >= 16 ? 4 : (NS >= 8 ? 3 : (NS >= 4 ? 2 : 1));
    const int slot = l15 >> (4 - SPLITS);
    const bool writer = (l15 & ((1 << (4 - SPLITS)) - 1)) == 0;
    if (writer) {
        const int co = (slot >> 2) * 16 + (slot & 3);
        sp[co] = 16.f * NV;
        sp[N + co] = m[0];
        sp[2 * N + co] = q[0];
    }
}

} }  // namespace mmh::dev

// Epilogue of the fp32 7x7 stem kernels that hold an 8 MT rows x 16 pixels x 64 channels output tile as MT 32x32 MFMA
// accumulators per wave (conv_stem_f32.hip's layout: wave = (pg = row pair, nh = channel half), lane = (m = channel, kg)):
// bias, activation, the store, and the (count, mean, M2) partials of the wave's 32 MT pixels per channel in the layout
// mmh_conv2d_fprop_stats_chunks describes.  The expressions are conv_stem_f32_kernel's, operation for operation: a kernel
// that reaches the same accumulators through this function writes the same bits.
// conv_stem_f32.hip does NOT include this header: it is the yardstick the sparse kernel is held against and stays as it was,
// with its own copy of these lines.  Nothing at compile time ties the two copies together; what does is
// tests/test_stem_sparse_gpu.py::test_sparse_fprop_is_the_dense_fprop_bit_for_bit, which compares y and the whole statistics
// buffer of the two kernels with torch.equal.  Change one copy and that test says so.
#pragma once
#include "device_prims.h"

namespace mmh { namespace dev {

template <int MT>
__device__ __forceinline__ void stem_f32_epilogue(const f32x16* acc, float* y, float* stats, int tile, int b, int ty, int tx,
                                                  int pg, int kg, int n, float bv, int H, int W, int y_cs, int act) {
    constexpr int TR = 8 * MT, TC = 16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        // acc[mt][i]: channel n, MFMA row (i & 3) + 8 (i >> 2) + 4 kg of tile rows 8 mt + 2 pg, + 1
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int mm = (i & 3) + 8 * (i >> 2) + 4 * kg;
            const int oh = ty * TR + 8 * mt + 2 * pg + (mm >> 4), ow = tx * TC + (mm & 15);
            if (oh < H && ow < W)
                y[((size_t)(b * H + oh) * W + ow) * (size_t)y_cs + n] = act_apply(acc[mt][i] + bv, act);
        }
    }
    if (stats) {
        // a lane holds 16 pixels of each accumulator tile, lane ^ 32 the other 16; Chan merges of equal counts
        float mean_w = 0.f, m2_w = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sum += acc[mt][i] + bv;
            const float mean_l = sum * (1.f / 16.f);
            float m2 = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float dv = acc[mt][i] + bv - mean_l;
                m2 += dv * dv;
            }
            const float mean_o = __shfl_xor(mean_l, 32, 64), m2_o = __shfl_xor(m2, 32, 64);
            const float dm = mean_o - mean_l;
            const float mean_t = mean_l + 0.5f * dm, m2_t = m2 + m2_o + dm * dm * 8.f;      // 32 pixels
            if (mt == 0) {
                mean_w = mean_t;
                m2_w = m2_t;
            } else {
                const float d2 = mean_t - mean_w;
                mean_w += 0.5f * d2;
                m2_w += m2_t + d2 * d2 * 16.f;                                              // 32 * 32 / 64
            }
        }
        if (kg == 0) {
            float* o = stats + ((size_t)(tile * 4 + pg) * 3) * 64 + n;
            o[0] = 32.f * MT;
            o[64] = mean_w;
            o[128] = m2_w;
        }
    }
}

} }  // namespace mmh::dev

// Shared host-side helpers, cross-file launcher declarations and option globals of libmmhand_hip.so (gfx950 only).
// Device primitives live in device_prims.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include "../../include/mmhand_hip.h"

namespace mmh {

// thread-local error text returned by mmh_last_error()
char* err_buf();
int fail(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
    return 0;
}

inline hipStream_t as_stream(mmh_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Winograd F(6x6,3x3) transforms (wino6.hip); tiles = B * ceil(H/6) * ceil(W/6), 64 planes
int wino6_weights(const float* w, float* U, int Cin, int Cout, int flip_transpose, hipStream_t st);
int wino6_weights_multi(const long long* table, int n, long long total_blocks, hipStream_t st);
int wino6_input(const float* x, float* V, int B, int H, int W, int C, int reflect, int xcd, hipStream_t st);
int wino6_output(const float* M, float* y, const float* bias, int B, int H, int W, int C, int act, float* stats,
                 int fold, hipStream_t st);
int wino6_dy(const float* dy, float* Yh, int B, int H, int W, int C, hipStream_t st);
int wino6_input_normact(const float* x, float* V, int B, int H, int W, int C, int reflect, int xcd,
                        const float* scale, const float* shift, int groups, int relu, float drop_p,
                        const uint32_t* drows, hipStream_t st);
int wino6_input_dy_normbwd(const float* g, const float* x, float* V, float* Yh, int B, int H, int W, int C, int xcd,
                           int fold, const float* mean, const float* invstd, const float* gamma, const float* s1,
                           const float* s2, double count, const float* scale, const float* shift,
                           const uint32_t* drows, int groups, int relu, float drop_p, hipStream_t st);
int wino6_input_dy(const float* dy, float* V, float* Yh, int B, int H, int W, int C, int xcd, int fold,
                   hipStream_t st);
int wino6_dw(const float* dU, float* dw, int Cin, int Cout, int accumulate, hipStream_t st);
// 16-bit wgrad of the 3x3 stride-1 stack with all nine taps resident (wgrad_lp16t.hip)
bool wgrad_lp16t_supported(const mmh_conv_desc* d);
int wgrad_lp16t_splits(const mmh_conv_desc* d);
int launch_wgrad_lp16t(const mmh_conv_desc* d, const void* x16, const void* dy16, float* slab, const void* zeros,
                       hipStream_t st);
// fp32 dgrad of the 3x3 stride-2 convs 64 -> 128 / 128 -> 256 with the dy halo resident in LDS (dgrad_s2.hip)
bool dgrad_s2_halo_ok(const mmh_conv_desc* d, int dx_cs, int act);
int launch_dgrad_s2_halo(const mmh_conv_desc* d, const void* dy, const void* w, const void* bias, void* dx, int dx_cs,
                         int act, hipStream_t st);
extern int g_dgrad_s2_halo, g_dgrad_s2_dbg;
// fp32 wgrad of the 3x3 stride-2 convs as a stream down a column strip of dy (wgrad_s2.hip)
bool wgrad_s2_strip_ok(const mmh_conv_desc* d);
size_t wgrad_s2_strip_ws_bytes(const mmh_conv_desc* d);
int launch_wgrad_s2_strip(const mmh_conv_desc* d, const void* x, const void* dy, void* dw, void* ws, size_t ws_bytes,
                          int accumulate, hipStream_t st);
extern int g_wgrad_s2_strip;
// fp32 fprop of the 7x7 stems from an LDS-resident input halo (conv_stem_f32.hip)
bool stem_f32_ok(const mmh_conv_desc* d);
int stem_f32_stats_chunks(const mmh_conv_desc* d);
int launch_stem_f32(const mmh_conv_desc* d, const void* x, const void* w, const void* bias, void* y, int act, float* stats,
                    hipStream_t st);
extern int g_stem_f32, g_stem_f32_dbg, g_stem_f32_levels;
// 1: the compacted-channel stem kernels answer "supported" (stem_sparse.hip), 0: every caller stays on the dense kernels
extern int g_stem_sparse;
// 1: D_PB's stem wgrad (the generic kernel's route) on stem_sparse_wgrad_flat_kernel where a mask exists, 0: stays dense
extern int g_stem_sparse_flat;
// the generic fp32 wgrad's split-K rule (conv_igemm.hip, do_wgrad): split s owns the flat dy-domain pixels
// [s * pix_per_split, min(P, (s + 1) * pix_per_split)), pix_per_split a multiple of its 32-pixel k-step
void wgrad_flat_split(int Mrows, int N, int P, int& splits, int& pix_per_split);
// fp32 Winograd-domain wgrad GEMMs as a three-stage LDS-DMA ring (wino_wgrad_dma.hip)
bool wino_wgrad_dma_ok(int64_t tiles, int Cin, int Cout, int nbatch);
size_t wino_wgrad_dma_ws_bytes(int64_t tiles, int Cin, int Cout, int nbatch);
int launch_wino_wgrad_dma(const float* V, const float* Yh, int64_t tiles, int Cin, int Cout, int nbatch, float* ws, float* dU,
                          hipStream_t st);
extern int g_wino_wgrad_dma;
// dw[b][i] (+)= sum over a batch's split-K slabs, fixed order (slab_reduce.hip)
int launch_slab_reduce(const float* slab, float* dw, int64_t n4_total, int splits, int accumulate, int64_t n4, hipStream_t st);
// 16-bit fprop of the 3x3 stride-2 convs with register-resident weights and an LDS-resident input halo (conv_s2_lp16.hip)
bool conv_s2f_ok(const mmh_conv_desc* d, int mode);
bool conv_s1f_ok(const mmh_conv_desc* d, int mode);     // its stride-1 form: 64 -> 64, zero padding, mode 0 fprop | 1 dgrad
int conv_s2f_stats_chunks(const mmh_conv_desc* d);
int launch_conv_s2f(const mmh_conv_desc* d, const void* x16, const void* w16, const void* bias, void* y, int y_is16, int act,
                    const void* zeros, hipStream_t st, float* stats = nullptr, int mode = 0);
bool conv_s2d_ok(const mmh_conv_desc* d, int mode);
int launch_conv_s2d(const mmh_conv_desc* d, const void* g16, const void* w16, const void* bias, void* dx, int dx_is16, int act,
                    const void* zeros, hipStream_t st);
extern int g_lp16_s2f;
extern int g_lp16_persist;
extern int g_slab_reduce_par;
extern int g_wino6_vec;
extern int g_lp16_shape;
extern int g_lp16_tap_inner;
extern int g_lp16_dbg;
extern int g_lp16_wgrad_ring;
extern int g_lp16_wgrad_s2;     // 1: the stride-2 3x3 wgrads on the nine-tap halo kernel (wgrad_lp16t.hip), 0: flat rows
extern int g_pw_v2;
extern int g_col_chunks, g_row_chunks;   // workgroups per launch the column-reduce / row kernels aim for

}  // namespace mmh

#define MMH_REQUIRE(cond, ...)                      \
    do {                                            \
        if (!(cond)) return mmh::fail(__VA_ARGS__); \
    } while (0)

/*
 * mmhand_hip.h — C-ABI of libmmhand_hip.so (MI355X / gfx950 only).
 *
 * The reference (VITA-Group/mm-hand) has no FFI of its own: its hot path,
 * MMHandModel.optimize_parameters() (models/MMHandModel.py:310-330), reaches
 * the GPU only through torch.nn modules.  This header therefore declares the
 * operator set those modules imply; every entry point
 * names the reference call site it replaces.
 *
 * Conventions
 *  - Activations are NHWC fp32 in HBM: element (b,h,w,c) of a tensor with
 *    channel stride `cs` sits at ((b*H + h)*W + w)*cs + c.  Channel counts are
 *    multiples of 4 (callers zero-pad 3/6/42-channel tensors to 4/8/44).
 *  - Conv weights are [kh][kw][Cin][Cout] ("RSCK", Cout contiguous) for Conv2d
 *    and [kh][kw][Cout_T][Cin_T] for ConvTranspose2d — the same physical
 *    object as the Conv2d whose dgrad the transposed conv is.
 *  - All device buffers are owned by the caller.  Nothing here allocates,
 *    frees or synchronises; every call enqueues on the caller's hipStream_t.
 *  - Return value: 0 on success, non-zero on error (mmh_last_error() gives the
 *    thread-local message).  No exceptions cross this boundary.
 */
#ifndef MMHAND_HIP_H
#define MMHAND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the entry points declared between this push and
 * the pop at the end of the header are its ONLY exported symbols (tests/test_host_cpu.py checks
 * `nm -D` against this header in both directions). */
#pragma GCC visibility push(default)

typedef void* mmh_stream_t; /* a hipStream_t */

enum { MMH_PAD_ZERO = 0, MMH_PAD_REFLECT = 1 };
enum { MMH_ACT_NONE = 0, MMH_ACT_RELU = 1, MMH_ACT_TANH = 2 };
enum { MMH_F32 = 0, MMH_BF16 = 1, MMH_FP16 = 2 };

/* Geometry of one Conv2d (forward orientation).  For ConvTranspose2d fill it
 * in as the Conv2d whose input-gradient the transposed conv computes. */
typedef struct mmh_conv_desc {
    int32_t B, H, W;      /* input  (x)  batch and spatial size            */
    int32_t Cin, Cout;    /* channels of w ([kh][kw][Cin][Cout]); %4 == 0   */
    int32_t kh, kw;       /* 3x3 or 7x7 in the reference                    */
    int32_t stride;       /* 1 or 2                                         */
    int32_t pad;          /* symmetric padding                              */
    int32_t pad_mode;     /* MMH_PAD_ZERO | MMH_PAD_REFLECT (stride 1 only) */
    int32_t Ho, Wo;       /* output (y) spatial size                        */
    int32_t x_cs, y_cs;   /* channel strides of x and y buffers (>= C)      */
    int32_t dtype;        /* MMH_F32, or MMH_BF16 / MMH_FP16 = 16-bit MFMA  */
                          /* operands (bf16, or IEEE fp16 as apex O1 uses), */
                          /* fp32 accumulation.  What is 16-bit IN HBM is   */
                          /* said per entry point: the first-generation     */
                          /* kernels (mmh_conv2d_*, mmh_convT2d_*) read     */
                          /* fp32 x / dy and round while staging unless     */
                          /* their io16 / lp16 argument says a tensor is    */
                          /* 16-bit; the conv_lp16 family (mmh_conv3x3_lp16,*/
                          /* mmh_conv_lp16, mmh_conv_lp16_flat, mmh_wgrad*  */
                          /* _lp16*) takes 16-bit x / dy and writes fp32 or */
                          /* 16-bit outputs (y_is16).  `w` is then a tensor */
                          /* made by mmh_prep_weights_bf16 / _fp16 (fprop / */
                          /* convT dgrad: w_t, or w_flat when Cin % 64 != 0;*/
                          /* dgrad / convT fprop: w_plain, Cout % 64 == 0). */
} mmh_conv_desc;

const char* mmh_last_error(void);
int mmh_version(void);
/* Tuning knobs for A/B measurements inside one process: kernel variants ("lp16_shape" 19 = the halo
 * kernel (default) | 17 = row tiles | 20 = one wave per SIMD (make AB=1 builds only), "lp16_wgrad_ring" 2 | 3,
 * "lp16_wgrad_s2" 0 | 1 (the stride-2 3x3 weight gradients on the flat-row kernel | on the nine-tap halo kernel,
 * default), "conv_dbuf",
 * "wino_gemm_levels", ...) and work-list parameters ("wgrad_slots", "conv_xcd", ...): the results
 * stay within the kernels' documented tolerances.  The "*_dbg" keys are NOT such knobs: "conv_dbg",
 * "lp16_dbg" (bits 1-16), "dgrad_s2_dbg", "stem_f32_dbg" switch parts of a kernel OFF for timing
 * ablations (tools/ablate*.py, tools/bench_lp16_fold.py) and make its results wrong ("lp16_dbg" bit 32 only
 * moves the DMA issue of half the waves, results unchanged: tools/ab_lp16_stagger.py); they default to 0
 * and nothing in mmhand_amd/ sets them.  Unknown keys are an error.
 * Every key (mmh_option_key enumerates the same list):
 *   fp32 implicit GEMM   "conv_dbuf" "conv_cw" "conv_bn256" "conv_levels" (1 | 2) "conv_xcd" "conv_xcd1" "conv_tall"
 *                        "dgrad_s2_multi" "dgrad_s2_halo" "border_bn64" "stem_f32"
 *                        "dgrad_levels" (1 | 2; 2: mmh_conv2d_dgrad's fp32 implicit GEMM with more than 64 input channels sums
 *                        every 32 of the (tap, channel) index in a chain of its own and adds the chains, as "conv_levels" 2
 *                        does for the forward; the 3D estimator's trainer sets it for its backward and puts it back)
 *   sparse fp32 stems    "stem_sparse" (1: the mmh_conv7_stem_sparse_*_supported queries may say yes, 0: they say no and
 *                        every caller stays on the dense kernels - the forward is bit-identical either way)
 *                        "stem_sparse_flat" (0: only mmh_conv7_stem_sparse_wgrad_flat_supported says no)
 *   fp32 wgrad           "wgrad_slots" "wgrad_dbuf" "wgrad_bn256" "wgrad_xcd" "wgrad_s2_strip" "slab_reduce_par"
 *   fp32 Winograd        "wino_bn256" "wino_xcd" "wino_gemm_v2" "wino_gemm_occ" "wino_gemm_bn" "wino_gemm_levels"
 *                        "wino_bf16_bk" "wino_bf16_occ" "wino6_vec" "wino_wgrad_v2" "wino_wgrad_occ"
 *                        "wino_wgrad_bn256" "wino_wgrad_slots" "wino_wgrad_dma"
 *   16-bit kernels       "lp16_shape" "lp16_s2f" "lp16_persist" "lp16_tap_inner" "lp16_wgrad_ring" "lp16_wgrad_s2"
 *   pointwise            "pw_v2" "col_chunks" "row_chunks" (the last two: values > 0 only)
 *   ablation switches    "conv_dbg" "lp16_dbg" "dgrad_s2_dbg" "stem_f32_dbg"                                  */
int mmh_set_option(const char* key, int value);
/* The current value of a key (to restore it after an A/B); unknown keys are an error. */
int mmh_get_option(const char* key, int* value);
/* The index-th key of the list above, NULL past its end. */
const char* mmh_option_key(int index);

/* ---- convolutions: nn.Conv2d / nn.ReflectionPad2d / nn.ConvTranspose2d ----
 * replaces models/Generator.py:40-113,158-259, models/Discriminator.py:14-99,
 * losses/L1_plus_perceptualLoss.py:22-27 (cuDNN kernels behind torch.nn).   */

/* y = act(conv(pad(x), w) + bias).  bias may be NULL. */
int mmh_conv2d_fprop(const mmh_conv_desc* d, const void* x, const void* w,
                     const void* bias, void* y, int act, mmh_stream_t s);

/* mmh_conv2d_fprop (fp32, no activation) that also writes, per (128-row tile, wave row) of the output GEMM,
 * the count / mean / M2 of every output column: stats [chunks][3][Cout], chunks =
 * mmh_conv2d_fprop_stats_chunks(d) (0: not available - B*Ho*Wo % 128 != 0 or a 16-bit dtype).  The norm
 * behind the conv (models/Generator.py:158-175 stems and down convs) merges them with
 * mmh_norm_stats_merge[_finalize] instead of reading y again; consecutive chunks cover consecutive pixels, so
 * with Ho*Wo % 128 == 0 the chunks of an image are contiguous (InstanceNorm: groups = B).              */
int mmh_conv2d_fprop_stats_chunks(const mmh_conv_desc* d);
int mmh_conv2d_fprop_stats(const mmh_conv_desc* d, const void* x, const void* w, const void* bias,
                           void* y, void* stats, mmh_stream_t s);
/* 1 when mmh_conv2d_dgrad / mmh_conv2d_dgrad_folded / mmh_convT2d_fprop run conv `d` (fp32, 3x3, stride 2,
 * zero pad 1, 64 -> 128 channels, dense dy) on the halo-resident kernel of dgrad_s2.hip - the 9 x 17 dy halo of
 * an 8 x 16 block of dy positions in LDS for all nine taps and all four output parity classes - instead of the
 * four parity-class implicit GEMMs (mmh_set_option("dgrad_s2_halo", 0) forces those).  Replaces the data
 * gradient of nn.Conv2d(ngf, 2 ngf, 3, 2, 1), models/Generator.py:192-199, and the forward of
 * nn.ConvTranspose2d(2 ngf, ngf, 3, 2, 1, output_padding=1), models/Generator.py:212-219.                      */
int mmh_dgrad_s2_halo_supported(const mmh_conv_desc* d, int dx_cs);

/* Gradient w.r.t. x.  MMH_PAD_ZERO: dx is [B,H,W,Cin] (channel stride
 * dx_cs).  MMH_PAD_REFLECT: dx is the gradient on the padded domain,
 * [B,H+2p,W+2p,Cin]; fold it with mmh_reflect_fold.                        */
int mmh_conv2d_dgrad(const mmh_conv_desc* d, const void* dy, const void* w,
                     void* dx, int dx_cs, mmh_stream_t s);

/* Gradient w.r.t. x, already folded back onto [B,H,W,Cin] for either pad mode.  For the
 * 3x3 / pad 1 reflect convs (the PATBlock / ResnetBlock stack) no padded buffer exists: a
 * tile-aligned zero-pad dgrad on the real domain plus one multi-piece launch that adds the
 * eight border terms of the pad ring.  Larger reflect pads go through `ws`
 * (mmh_conv2d_dgrad_folded_ws_bytes) and mmh_reflect_fold.                       */
size_t mmh_conv2d_dgrad_folded_ws_bytes(const mmh_conv_desc* d);
int mmh_conv2d_dgrad_folded(const mmh_conv_desc* d, const void* dy, const void* w,
                            void* dx, void* ws, size_t ws_bytes, mmh_stream_t s);

/* ---- Winograd for the fp32 3x3 / stride 1 / pad 1 convs (the PATBlock / ResnetBlock stack) ----
 * y = A^T[(G g G^T) . (B^T d B)]A with tile = 2 (F(2x2,3x3): 16 planes, 2.25x fewer
 * multiplications than the direct implicit GEMM), tile = 4 (F(4x4,3x3): 36 planes, 4x fewer;
 * fp32 error 2.4e-6 relative at K = 512) or tile = 6 (F(6x6,3x3): 64 planes, 5.06x fewer, 5e-6;
 * ragged tiles: any H, W >= 4).  tiles = B*ceil(H/tile)*ceil(W/tile) (tile 2, 4: H, W % tile
 * == 0); planes P = (tile+2)^2.
 *   U  [P][K][N]     = mmh_wino_weights(w)  (flip_transpose=1: the dgrad filter [P][Cout][Cin])
 *   V  [P][tiles][C] = mmh_wino_input(x)    (reflect or zero padding folded into the gather)
 *   M  [P][tiles][N] = mmh_wino_gemm(V, U)  (P batched GEMMs, one launch)
 *   y                = mmh_wino_output(M)   (+bias, activation)
 * dgrad: the same three stages on dy with zero padding and the flipped filter give g on the
 *        real domain; mmh_conv2d_dgrad_border adds the eight reflect-border terms.
 * wgrad: Yh = mmh_wino_dy(dy) = A dY A^T; dU = mmh_wino_wgrad_gemm(V, Yh) (P split-K GEMMs over
 *        the tiles, deterministic slab reduction); dw = mmh_wino_dw(dU) = G^T dU G.
 * dtype = MMH_F32: every Winograd-domain tensor is fp32 (tile 2 or 4).
 * dtype = MMH_BF16 (tile 2 only; the --opt_level O1/O2 path): U, V, M and Yh are bf16 in HBM,
 *        transforms compute in fp32 and round once, the GEMMs run on the bf16 MFMA with fp32
 *        accumulation; x, y, dy, dU, dw, bias stay fp32.  bf16 U is [P][N][K] (contraction index
 *        contiguous).  Needs K % 64 == 0, N % 32 == 0 (wgrad: Cin, Cout % 128 == 0).        */
int mmh_wino_weights(const void* w, int Cin, int Cout, int flip_transpose, int tile, int dtype,
                     void* U, mmh_stream_t s);
/* reflect: 0 = zero padding 1, 1 = reflection padding 1, 2 (tile 6, fp32) = zero padding 2 with
 * tiles over the (H+2) x (W+2) outputs of the full correlation: the first stage of the
 * REFLECT-FOLD dgrad.  The gradient of a ReflectionPad2d(1) conv lives on the padded domain and
 * its transpose adds ring row -1 onto row 1 and ring row H onto row H-2; with the tile origin on
 * the ring, each ring pixel and its partner sit in one 6x6 tile, so mmh_wino_output(fold=1) adds
 * them in registers: dgrad costs the same 64 GEMMs as fprop and no border terms.  Needs
 * (H+1) % 6 >= 2 and (W+1) % 6 >= 2 (true for 16, 64, 128: the shapes of the path); tiles =
 * B*ceil((H+2)/6)*ceil((W+2)/6).                                                           */
int mmh_wino_input(const void* x, int B, int H, int W, int C, int reflect, int tile, int dtype,
                   void* V, mmh_stream_t s);
int mmh_wino_dy(const void* dy, int B, int H, int W, int C, int tile, int dtype, void* Yh,
                mmh_stream_t s);
/* Both backward transforms of dy in one pass (tile 6, fp32): V = mmh_wino_input(dy, zero pad) for
 * the dgrad GEMMs and Yh = mmh_wino_dy(dy) for the wgrad GEMMs; dy is read once.
 * fold != 0: V is taken on the padded domain as mmh_wino_input(reflect=2) does (needs, besides
 * its conditions, ceil((H+2)/6) == ceil(H/6) so that V and Yh share one tile grid).           */
int mmh_wino_input_dy(const void* dy, int B, int H, int W, int C, int tile, int dtype, void* V,
                      void* Yh, int fold, mmh_stream_t s);
int mmh_wino_gemm(const void* V, const void* U, void* M, int64_t tiles, int K, int N,
                  int nbatch, int dtype, mmh_stream_t s);
/* The fp32 GEMMs with the summation chosen per call: levels = 2 folds every 32-deep k-step's chain into the
 * totals (the default of mmh_wino_gemm for 64 planes: the F(6x6,3x3) output transform amplifies the rounding of
 * one k-ordered chain), levels = 1 is one chain (5-6 % faster).  The package runs the FORWARD GEMMs with 2 and
 * the dgrad GEMMs with 1: a forward difference of 7e-6 flips ReLU masks and moves the parameter gradients of
 * this network by 3e-3, a backward one cannot (profiles/r03_wino_grad_split.txt: Winograd dgrad alone 6e-6).  */
int mmh_wino_gemm_levels(const void* V, const void* U, void* M, int64_t tiles, int K, int N,
                         int nbatch, int levels, mmh_stream_t s);
/* The 16 Winograd-domain GEMMs of F(2x2,3x3) (V [16][tiles][K], U [16][K][N] -> M [16][tiles][N], fp32) with the
 * summation chosen per call.  levels = 2: a fresh MFMA chain per 32-deep k-step, folded into the totals by vector adds -
 * the definition of the direct two-level fprop and of the 64-plane GEMMs - which mmh_wino_gemm_levels never runs for
 * 16 planes (it folds 64 planes only and keeps doing so).  Fixed summation order, no atomics; a tile's result does not
 * depend on the number of tiles.  Needs K % 32 == 0, N % 32 == 0, N >= 64.  Between mmh_wino_input(tile 2) and
 * mmh_wino_output(tile 2) it is the forward of ops.set_winograd_mode("bwd_f2") for the 3x3 stride-1 convs of the
 * reference's PATBlock conv stack (models/Generator.py:40-113).                                                       */
int mmh_wino_gemm_levels16(const void* V, const void* U, void* M, int64_t tiles, int K, int N, int levels,
                           mmh_stream_t s);
/* The F(6x6,3x3) filter transform of MANY fp32 filters in one launch (after an optimizer step a network's 74
 * transforms are 8-25 us launches that cannot fill the chip).  table: n rows of six int64 in device memory -
 * {w pointer, U pointer, Cin, Cout, flip_transpose, first block} - entry e owning the 256-thread blocks
 * [first block of e, first block of e + 1), ceil(Cin Cout / 256) of them; total_blocks their sum.  Each entry
 * gets exactly what mmh_wino_weights(w, Cin, Cout, flip_transpose, 6, MMH_F32, U) writes.                  */
int mmh_wino_weights_multi(const void* table, int n, int64_t total_blocks, mmh_stream_t s);
/* stats (tile 6, fp32; may be NULL): [B][tiles per image][3][C] floats = per (image, tile, channel)
 * the count, mean and M2 of the tile's outputs - the partial-statistics layout that
 * mmh_norm_stats_merge reduces, so the InstanceNorm after the conv does not re-read y.
 * fold != 0 (tile 6, fp32, no bias / act / stats): M is on the padded domain (see mmh_wino_input,
 * reflect = 2); y receives the reflect-folded gradient on the real H x W domain.               */
int mmh_wino_output(const void* M, void* y, const void* bias, int B, int H, int W, int C,
                    int act, int tile, int dtype, void* stats, int fold, mmh_stream_t s);
size_t mmh_wino_wgrad_gemm_ws_bytes(int64_t tiles, int Cin, int Cout, int nbatch);
int mmh_wino_wgrad_gemm(const void* V, const void* Yh, int64_t tiles, int Cin, int Cout,
                        int nbatch, int dtype, void* ws, size_t ws_bytes, void* dU,
                        mmh_stream_t s);
int mmh_wino_dw(const void* dU, int Cin, int Cout, int tile, void* dw, int accumulate,
                mmh_stream_t s);
size_t mmh_conv2d_dgrad_border_ws_bytes(const mmh_conv_desc* d);
/* phase 1 = the eight border GEMMs (dy, w -> ws; independent of dx, so the caller may run
 * them on a second stream beside the Winograd transforms), 2 = add ws into dx, 3 = both.
 * io16: bit 0 = dy, bit 1 = dx is a 16-bit tensor of d->dtype (gradients of a 16-bit convolution). */
int mmh_conv2d_dgrad_border(const mmh_conv_desc* d, const void* dy, const void* w, void* dx,
                            void* ws, size_t ws_bytes, int phase, int io16, mmh_stream_t s);

/* dw[kh][kw][Cin][Cout] (+)= sum over pixels.  Split-K partial slabs go to
 * `ws` (mmh_conv2d_wgrad_ws_bytes); the fixed-order second stage makes the
 * result deterministic.  accumulate!=0 adds into dw.                       */
size_t mmh_conv2d_wgrad_ws_bytes(const mmh_conv_desc* d);
/* io16 (16-bit dtypes): 0 = x and dy are fp32 (converted on load), 3 = both are already 16-bit in HBM. */
int mmh_conv2d_wgrad(const mmh_conv_desc* d, const void* x, const void* dy,
                     void* dw, void* ws, size_t ws_bytes, int accumulate,
                     int io16, mmh_stream_t s);

/* ConvTranspose2d(k3,s2,p1,op1) (models/Generator.py:240-253).  `d` is the
 * stride-2 Conv2d of which this is the dgrad: d->{H,W,Cin} describe the
 * transposed conv's OUTPUT, d->{Ho,Wo,Cout} its INPUT.                     */
int mmh_convT2d_fprop(const mmh_conv_desc* d, const void* x, const void* w,
                      const void* bias, void* y, int y_cs, int act,
                      mmh_stream_t s);
int mmh_convT2d_dgrad(const mmh_conv_desc* d, const void* dy, const void* w,
                      void* dx, mmh_stream_t s);
int mmh_convT2d_wgrad(const mmh_conv_desc* d, const void* x, const void* dy,
                      void* dw, void* ws, size_t ws_bytes, int accumulate,
                     int io16, mmh_stream_t s);

/* fp32 weights [taps][Cin][Cout] -> bf16 copies for the MMH_BF16 conv path:
 * w_plain [taps][Cin][Cout] (contraction = Cout, used by dgrad) and
 * w_t [taps][Cout][Cin] (contraction = Cin, used by fprop).  Either may be NULL. */
int mmh_prep_weights_bf16(const void* w, int taps, int Cin, int Cout,
                          void* w_plain, void* w_t, mmh_stream_t s);
/* The same two copies as IEEE fp16 (MMH_FP16; values beyond +-65504 become inf).          */
int mmh_prep_weights_fp16(const void* w, int taps, int Cin, int Cout,
                          void* w_plain, void* w_t, mmh_stream_t s);
/* Both copies of MANY weights in one launch (after an optimizer step every 16-bit copy of a network is stale: 78
 * conversions of 5-15 us per 16-bit iteration).  table: n rows of eight int64 in device memory - {w pointer, w_plain
 * pointer, w_t pointer (either copy may be 0), taps, Cin, Cout, first block, 1 for fp16 | 0 for bf16} - entry e owning
 * the 256-thread blocks [first block of e, first block of e + 1), taps ceil(Cin / 64) ceil(Cout / 64) of them; total_blocks
 * their sum.  Each entry gets exactly what mmh_prep_weights_bf16 | _fp16 writes.  The optimizer the reference steps
 * (models/MMHandModel.py:317-330, apex O1 casting weights per forward) is where the copies go stale.           */
int mmh_prep_weights_lp16_multi(const void* table, int n, int64_t total_blocks, mmh_stream_t s);
int mmh_prep_weights_fp16_flat(const void* w, int taps, int Cin, int Cout,
                               void* w_flat, mmh_stream_t s);
/* For fprop of convs whose Cin is not a multiple of 64 (the 7x7 stems): w_flat is
 * [Cout][Kpad] bf16, Kpad = ceil(taps*Cin/64)*64, contraction index k = tap*Cin + ci. */
int mmh_prep_weights_bf16_flat(const void* w, int taps, int Cin, int Cout,
                               void* w_flat, mmh_stream_t s);

/* Diagnostic builds only (make AB=1; mmh_set_option("lp16_dbg", 4096)): after launches of the 16-bit halo kernel, copies
 * per workgroup the pair (delta s_memtime, delta s_memrealtime) that wave 0 stamped around the kernel body into
 * host_pairs_u64[2 * max_workgroups]; delta s_memtime / delta s_memrealtime x 100 MHz is the clock the chip held under the
 * kernel's load.  Synchronises the device.  Returns the number of workgroups copied: 0 in ordinary builds (no stamp is
 * compiled into the shipped kernel), -1 on a copy error.                                                                */
int mmh_lp16_clock_stamps(void* host_pairs_u64, int max_workgroups);

/* ---- 16-bit direct 3x3 convolution, both operands 16-bit in HBM (conv_lp16.hip) ----------------
 * The second-generation MFMA kernel of the --opt_level O1/O2 path for the 3x3 / stride 1 / pad 1
 * stack (channels % 64 == 0, output channels % 256 == 0): 256x256x64 block tile, both operands
 * global -> LDS by LDS-DMA with an XOR-swizzled image, two 64 KiB stages, one barrier per k-step.
 *   x16   16-bit NHWC activations (the twin of the fp32 tensor: mmh_cvt_lp16, or written by the
 *         producer), pixel stride d->x_cs (mode 0) / d->y_cs (mode 1) elements
 *   w16   mode 0 (fprop): w_t [tap][Cout][Cin]; mode 1 (dgrad): w_plain [tap][Cin][Cout]
 *         (mmh_prep_weights_bf16 / _fp16)
 *   y     fp32 (y_is16 = 0) or 16-bit (y_is16 = 1) NHWC output, +bias, activation
 *   zeros >= 128 zero bytes of device memory (what out-of-image taps read)
 * mode 1 computes the zero-padded correlation with the flipped filter; for MMH_PAD_REFLECT the
 * caller adds the border terms (mmh_conv2d_dgrad_border, phase 3) afterwards.
 * mmh_wgrad3x3_lp16: dw [3][3][Cin][Cout] fp32 (+)= wgrad from the 16-bit x and dy (Cin, Cout
 * % 256 == 0): [64 pixels][256 channels] tiles by LDS-DMA, both MFMA operands read transposed
 * (ds_read_b64_tr_b16), split-K over pixel ranges with fp32 slabs in ws, fixed-order reduction.  */
int mmh_cvt_lp16(const void* x, int64_t n, int dtype, void* out, mmh_stream_t s);
size_t mmh_wgrad3x3_lp16_ws_bytes(const mmh_conv_desc* d);
int mmh_wgrad3x3_lp16(const mmh_conv_desc* d, const void* x16, const void* dy16, void* dw,
                      void* ws, size_t ws_bytes, int accumulate, const void* zeros,
                      mmh_stream_t s);
int mmh_conv3x3_lp16_supported(const mmh_conv_desc* d);
/* mode 2 of mmh_conv3x3_lp16: the dgrad of a ReflectionPad2d(1) conv complete in one launch -
 * the gradient of the pad ring is folded onto rows 1 / H-2 and columns 1 / W-2 inside the halo
 * kernel (H, W multiples of 16, Cin % 256 == 0), so no mmh_conv2d_dgrad_border call follows.     */
int mmh_conv3x3_lp16_fold_supported(const mmh_conv_desc* d);
int mmh_conv3x3_lp16(const mmh_conv_desc* d, int mode, const void* x16, const void* w16,
                     const void* bias, void* y, int y_is16, int act, const void* zeros,
                     mmh_stream_t s);
/* fprop (16-bit y, no activation) that also writes the partial statistics of its output from the
 * epilogue: stats [B][chunks][3][Cout] floats = count / mean / M2 per (image, half pixel tile,
 * channel) of the values as stored - the mmh_norm_stats_merge[_finalize] layout, so the InstanceNorm
 * behind the conv (models/Generator.py:66-77) does not read y for statistics.  chunks =
 * mmh_conv3x3_lp16_stats_chunks(d) = 2 (H/16)(W/16); 0 = not available (H or W not a multiple of 16). */
/* dgrad (mode 1 | 2) of the 3x3 stack with a 16-bit dx that is the gradient of a norm's OUTPUT (conv -> norm -> ReLU ->
 * Dropout -> pad -> conv, models/Generator.py:66-77, models/Discriminator.py:35-48): the epilogue also takes that norm's
 * backward sums s1 = sum dz, s2 = sum dz * xhat per (group, channel) - dz = keep ? g * dsc : 0 of the values as stored -
 * as partials per (image, half tile) in ws, which mmh_norm_bwd_sums_final adds up: mmh_norm_bwd_reduce's pass over g, x
 * and the keep bits is gone.  xn: the norm's input, 16-bit [B,H,W,Cin] contiguous; bits: its keep bits (16 per 8
 * elements, mmh_scale_shift_act's) or NULL; mean / invstd fp32 [groups][Cin], groups = B (InstanceNorm) | 1
 * (BatchNorm); s1 / s2 fp32 [groups][Cin]; ws >= B * chunks * 2 * Cin floats, 16-byte aligned.
 * _chunks: partials per image, 0 = not available (ragged tiles, strided dx, another kernel selected).               */
int mmh_conv3x3_lp16_dgrad_nbr_chunks(const mmh_conv_desc* d, int mode);
int mmh_conv3x3_lp16_dgrad_nbr(const mmh_conv_desc* d, int mode, const void* dy16, const void* w16, void* dx16,
                               const void* xn, const void* bits, const void* mean, const void* invstd, int groups,
                               float drop_p, void* s1, void* s2, void* ws, size_t ws_bytes, const void* zeros,
                               mmh_stream_t s);
/* partials [groups][chunks][2][C] -> s1, s2 [groups][C]: the second half of mmh_norm_bwd_reduce alone */
int mmh_norm_bwd_sums_final(const void* part, int groups, int C, int chunks, void* s1, void* s2, mmh_stream_t s);

/* dgrad (mode 1 | 2) with an fp32 dx that also receives `addend` (fp32, same layout as dx) in the epilogue:
 * dx = dgrad(dy) + addend.  The conv's input has a second consumer - the residual stream of a PATBlock
 * (models/Generator.py:115-130) or a ResnetBlock (models/Discriminator.py:50) - whose gradient
 * autograd would otherwise add in a pass of its own (35 launches, 1.7 ms per 16-bit step).        */
int mmh_conv3x3_lp16_dgrad_add_supported(const mmh_conv_desc* d);
int mmh_conv3x3_lp16_dgrad_add(const mmh_conv_desc* d, int mode, const void* dy16, const void* w16,
                               const void* addend, void* dx, const void* zeros, mmh_stream_t s);
int mmh_conv3x3_lp16_stats_chunks(const mmh_conv_desc* d);
int mmh_conv3x3_lp16_fprop_stats(const mmh_conv_desc* d, const void* x16, const void* w16,
                                 const void* bias, void* y16, void* stats, const void* zeros,
                                 mmh_stream_t s);

/* The same machine for the other 3x3 / pad 1 convolutions of the step (stride 2 down-sampling,
 * ConvTranspose2d, 64 / 128 output channels): mode 0 fprop, mode 1 dgrad (stride 2: the four
 * output-parity classes in one launch; ConvTranspose2d(k3,s2,p1,op1).forward is mode 1 of the
 * stride-2 conv it is the adjoint of).  Needs Cin, Cout % 64 == 0, even H and W for stride 2.
 * Operands as for mmh_conv3x3_lp16.  models/Generator.py:165-223,240-253, Discriminator.py:86-99. */
int mmh_conv_lp16_supported(const mmh_conv_desc* d, int mode);
int mmh_conv_lp16(const mmh_conv_desc* d, int mode, const void* x16, const void* w16,
                  const void* bias, void* y, int y_is16, int act, const void* zeros,
                  mmh_stream_t s);
/* fprop (mode 0) with a 16-bit output AND the partial statistics of that output for the InstanceNorm behind the conv,
 * where the stride-2 kernel of conv_s2_lp16.hip takes the shape (3x3 / stride 2 / zero pad 1, Cin 64, Cout %% 128 == 0,
 * Ho %% 8 == 0, Wo %% 16 == 0): stats [B][chunks][3][Cout], chunks = mmh_conv_lp16_stats_chunks(d) (0: use
 * mmh_conv_lp16 and mmh_norm_stats).                                                                                  */
int mmh_conv_lp16_stats_chunks(const mmh_conv_desc* d);
int mmh_conv_lp16_fprop_stats(const mmh_conv_desc* d, const void* x16, const void* w16, const void* bias, void* y16,
                              void* stats, const void* zeros, mmh_stream_t s);

/* Flat-K 16-bit fprop for the 7x7 stems (Cin = 3..42: models/Generator.py:158-164,
 * models/Discriminator.py:79-84): contraction index k = tap * C8 + c over the channels padded to C8
 * (a multiple of 8, <= 64).  x16p = mmh_lp16_pad_cvt(x) [B][H][W][C8]; w_flat =
 * mmh_prep_weights_lp16_flat8(w) [Cout][roundup(kh*kw*C8, 64)]; stride 1, 'same' zero / reflect padding. */
int mmh_lp16_pad_cvt(const void* x, int64_t rows, int C, int C8, int dtype, void* out, mmh_stream_t s);
int mmh_prep_weights_lp16_flat8(const void* w, int taps, int Cin, int Cout, int C8, int dtype,
                                void* out, mmh_stream_t s);
int mmh_conv_lp16_flat_supported(const mmh_conv_desc* d, int C8);
int mmh_conv_lp16_flat(const mmh_conv_desc* d, const void* x16p, int C8, const void* w_flat,
                       const void* bias, void* y, int y_is16, int act, const void* zeros,
                       mmh_stream_t s);

/* 16-bit wgrad with flat (tap, channel) rows - the stems, the stride-2 convs and ConvTranspose2d under
 * apex O1 (models/Generator.py:158-223,240-253, models/Discriminator.py:79-99): dw [kh][kw][Cin][Cout]
 * fp32 (+)= from x16 [B][H][W][x_cs] (C8 channels per tap read: C8 = Cin, or the padded width of
 * mmh_lp16_pad_cvt) and dy16 [B][Ho][Wo][y_cs].  ConvTranspose2d: x16 := its output gradient, dy16 :=
 * its input, d = the stride-2 conv it is the adjoint of (as mmh_convT2d_wgrad).              */
int mmh_wgrad_lp16_flat_supported(const mmh_conv_desc* d, int C8);
size_t mmh_wgrad_lp16_flat_ws_bytes(const mmh_conv_desc* d, int C8);
int mmh_wgrad_lp16_flat(const mmh_conv_desc* d, const void* x16, int C8, int x_cs, const void* dy16,
                        void* dw, void* ws, size_t ws_bytes, int accumulate, const void* zeros,
                        mmh_stream_t s);

/* 16-bit fprop of the same stems with the 22 x 22 pixel input halo of a 16 x 16 pixel tile resident in LDS and
 * the filter's column taps flattened into the contraction (conv_stem16.hip): the pixel fragment is read
 * straight from the flat halo row at pixel pitch C8, no im2col tile is staged (mmh_conv_lp16_flat moves 40 KB
 * per 64-deep k-step).  x16p [B,H,W,C8] as above; w_stem16 from mmh_prep_weights_stem16 (the stem's fp32
 * weight [7][7][Cin][64] as 16-bit [7][64][32 ceil(7 C8 / 32) + 8], mmh_conv_stem16_weights_bytes(C8) bytes);
 * y fp32 or 16-bit (y_is16) [B,H,W,y_cs], +bias, activation.                                         */
int mmh_conv_stem16_supported(const mmh_conv_desc* d, int C8);
size_t mmh_conv_stem16_weights_bytes(int C8);
/* the same kernel with a 3x3 / pad 1 filter at C8 == 8 (ks = 3; ks = 7: the functions above): VGG19's conv1_1 (3 -> 64 at
 * full resolution, losses/L1_plus_perceptualLoss.py:22-27) - mmh_conv_stem16 takes it from the descriptor's kh           */
size_t mmh_conv_stem16_weights_bytes_k(int C8, int ks);
int mmh_prep_weights_stem16_k(const void* w, int Cin, int C8, int ks, int dtype, void* out, mmh_stream_t s);
int mmh_prep_weights_stem16(const void* w, int Cin, int C8, int dtype, void* out, mmh_stream_t s);
int mmh_conv_stem16(const mmh_conv_desc* d, const void* x16p, int C8, const void* w_stem16,
                    const void* bias, void* y, int y_is16, int act, const void* zeros,
                    mmh_stream_t s);
/* The same launch also leaving the partial statistics of its 16-bit output for the InstanceNorm behind the stem
 * (H, W multiples of 16; no activation): stats [B][chunks][3][64] (n, mean, M2 per wave tile and channel) in the layout
 * mmh_norm_stats_merge_finalize reduces - the norm does not read y for statistics.  chunks = mmh_conv_stem16_stats_chunks
 * (0: not available for this shape).                                                                                  */
int mmh_conv_stem16_stats_chunks(const mmh_conv_desc* d, int C8);
int mmh_conv_stem16_stats(const mmh_conv_desc* d, const void* x16p, int C8, const void* w_stem16, const void* bias,
                          void* y16, void* stats, const void* zeros, mmh_stream_t s);

/* 16-bit wgrad of the 7x7 / stride 1 / pad 3 stems with 64 output channels (models/Generator.py:158-164,
 * models/Discriminator.py:60-64): x16p [B,H,W,C8] = the stem's 16-bit input with its channels padded
 * to C8 (mmh_lp16_pad_cvt; C8 % 8 == 0, 8..48), dy16 [B,H,W,y_cs >= 64].  The filter's column taps are
 * flattened into the operand (a row of the NHWC input is one contiguous array: the window of pixel
 * ow starts at element ow * C8), the contraction runs over the pixels of a row, both MFMA operands
 * are read transposed from an LDS halo staged once per 4 x 16 pixel block for all 49 taps; split-K
 * slabs in ws, summed in a fixed order.  dw [7][7][Cin][64] fp32 (+)= ...                          */
int mmh_wgrad_stem_lp16_supported(const mmh_conv_desc* d, int C8);
size_t mmh_wgrad_stem_lp16_ws_bytes(const mmh_conv_desc* d, int C8);
int mmh_wgrad_stem_lp16(const mmh_conv_desc* d, const void* x16p, int C8, const void* dy16, void* dw,
                        void* ws, size_t ws_bytes, int accumulate, const void* zeros,
                        mmh_stream_t s);

/* Weight gradient of the Generator head (ReflectionPad2d(3) + Conv2d(64, 3, 7) + Tanh, models/Generator.py:254-259;
 * Cout = 3 padded to 4) in 16 bits: d describes the head conv (Cin = 64, Cout = 4, reflect pad 3, dtype BF16 | FP16),
 * x16 = its 16-bit input [B,H,W,x_cs >= 64], dy = the fp32 gradient of its output [B,H,W,y_cs >= 4] (after the Tanh
 * backward).  dw[kh][kw][ci][co] = sum over q of the padded domain of xpad[q][ci] * E[q + (3-kh, 3-kw)][co] with E = dy
 * embedded at offset (3,3): the stem wgrad above on the padded domain with the roles of the operands swapped (E is the
 * 8-channel "input", the 64 channels of x the "output gradient", read through reflected source addresses), mirrored and
 * transposed by the slab reduction.  dw [7][7][64][4] fp32 (+)= ...; ws 16-byte aligned.  Replaces the fp32 vector-ALU
 * kernel mmh_conv7_thin_wgrad in 16-bit mode.                                                                        */
int mmh_conv7_head_wgrad_lp16_supported(const mmh_conv_desc* d);
size_t mmh_conv7_head_wgrad_lp16_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_head_wgrad_lp16(const mmh_conv_desc* d, const void* x16, const void* dy, void* dw, void* ws,
                              size_t ws_bytes, int accumulate, const void* zeros, mmh_stream_t s);

/* Transpose of ReflectionPad2d(p): dx[b,h,w,c] = sum of dxp over the padded
 * positions that mirror onto (h,w).  dxp is [B,H+2p,W+2p,C].               */
int mmh_reflect_fold(const void* dxp, void* dx, int B, int H, int W, int C,
                     int p, mmh_stream_t s);

/* out[c] (+)= sum over rows of x[rows][C] (conv-bias gradient).  x_dtype: element type of x
 * (MMH_F32 | MMH_BF16 | MMH_FP16); sums are fp32.                          */
size_t mmh_colsum_ws_bytes(int64_t rows, int C);
int mmh_colsum(const void* x, int64_t rows, int C, int cs, void* out,
               void* ws, size_t ws_bytes, int accumulate, int x_dtype, mmh_stream_t s);

/* ---- BatchNorm2d / InstanceNorm2d + ReLU + Dropout ------------------------
 * replaces norm_layer / nn.ReLU / nn.Dropout sites, models/Generator.py:66-77,
 * models/Discriminator.py:29-34, models/network_utils.py:74-84.
 * The *_dtype arguments name the element type of one activation / gradient tensor in HBM
 * (MMH_F32 | MMH_BF16 | MMH_FP16).  Under --opt_level O1 the tensors that face a convolution
 * (its output, its input, both gradients) are 16-bit, as under apex; statistics, scale / shift,
 * sums and all arithmetic stay fp32.                                        */

/* Per-(group,channel) mean and M2 = sum (x-mean)^2.  groups = B for instance
 * norm (rows_per_group = H*W), 1 for batch norm (rows_per_group = B*H*W).   */
size_t mmh_norm_stats_ws_bytes(int groups, int64_t rows_per_group, int C);
int mmh_norm_stats(const void* x, int groups, int64_t rows_per_group, int C,
                   int cs, void* mean, void* m2, void* ws, size_t ws_bytes,
                   int x_dtype, mmh_stream_t s);

/* Chan merge of `chunks` partial (count, mean, M2) triples per (group, channel), laid out
 * [groups][chunks][3][C] (what mmh_wino_output(stats) writes): the second stage of mmh_norm_stats. */
int mmh_norm_stats_merge(const void* partials, int groups, int chunks, int C, void* mean,
                         void* m2, mmh_stream_t s);

/* The same merge for ONE group over many chunks in two levels (BatchNorm statistics from conv-epilogue
 * partials, models/network_utils.py:74-84 with --norm batch: B * chunks-per-image partials per channel):
 * `sub` blocks of chunks (chunks % sub == 0) are merged in parallel into [sub][3][C] floats in ws, which
 * a single-group merge finishes.                                                                      */
size_t mmh_norm_stats_merge2_ws_bytes(int sub, int C);
int mmh_norm_stats_merge2(const void* partials, int chunks, int C, int sub, void* ws,
                          size_t ws_bytes, void* mean, void* m2, mmh_stream_t s);

/* mmh_norm_stats_merge + mmh_norm_finalize of a norm without affine parameters and running statistics
 * (nn.InstanceNorm2d) in one launch: the same fp32 mean / M2 / scale / shift / invstd as the two calls.   */
int mmh_norm_stats_merge_finalize(const void* partials, int groups, int chunks, int C, double count,
                                  float eps, void* mean, void* m2, void* scale, void* shift,
                                  void* invstd, mmh_stream_t s);
/* SyncBN (apex convert_syncbn_model, models/MMHandModel.py:109-116): the (count, mean, M2) triples of one norm site as the
 * ranks' all-gather delivered them - rank r's triple at gathered + r * rank_stride floats, [3][C] - merged in rank order
 * (Chan) AND finalised (affine, running statistics with momentum and the unbiased variance) in one launch: the same values as
 * mmh_norm_stats_merge on the [ranks][3][C] block followed by mmh_norm_finalize, without the block copy and the two launches.
 * count = rows over all ranks.                                                                                          */
int mmh_syncbn_merge_finalize(const void* gathered, int ranks, int64_t rank_stride, int C, double count,
                              float eps, const void* gamma, const void* beta, void* mean, void* m2,
                              void* scale, void* shift, void* invstd, void* running_mean,
                              void* running_var, float momentum, mmh_stream_t s);
/* scale = gamma*rsqrt(m2/count+eps), shift = beta - mean*scale, invstd.
 * gamma/beta may be NULL (affine=False).  If running_mean != NULL (batch
 * norm, groups==1) they are updated with momentum and the unbiased variance
 * m2/(count-1), as nn.BatchNorm2d does in training mode.                   */
int mmh_norm_finalize(const void* mean, const void* m2, double count,
                      const void* gamma, const void* beta, float eps,
                      int groups, int C, void* scale, void* shift,
                      void* invstd, void* running_mean, void* running_var,
                      float momentum, mmh_stream_t s);

/* out = dropout(relu(x*scale[g][c] + shift[g][c])) (+ residual).  scale and
 * shift are [groups][C].  Dropout keeps an element when a counter-based hash
 * of (seed, element position) clears the drop threshold and scales by 1/(1-p);
 * if mask != NULL (uint8 per element, test hook) it is used instead.
 * keep_bits != NULL (uint8 per 4 channels): bit e = lane e survived ReLU / dropout -
 * all the backward needs of `out`, at 1/16 of its bytes.
 * out_dtype: MMH_F32, or MMH_BF16 / MMH_FP16 = `out` is written as that 16-bit type
 * (the input of a 16-bit convolution: no fp32 copy, no conversion pass).      */
int mmh_scale_shift_act(const void* x, const void* scale, const void* shift,
                        const void* residual, void* out, int groups,
                        int64_t rows_per_group, int C, int relu, float drop_p,
                        uint64_t seed, const void* mask, void* keep_bits,
                        int x_dtype, int out_dtype, mmh_stream_t s);
/* The same pass writing `out` AND the same values in 16 bits to `twin` (twin_dtype MMH_BF16 | MMH_FP16): a norm output with
 * two consumers - the residual stream of a ResnetBlock (models/Discriminator.py:50), a PATBlock's first stream-1 input -
 * stays fp32 for the residual add, and the 3x3 conv that reads it takes the twin instead of a conversion pass of its
 * own (mmh_cvt_lp16: 6 B per element against 2).  Needs C / 8 a power of two <= 256.                                      */
int mmh_scale_shift_act_twin(const void* x, const void* scale, const void* shift,
                             const void* residual, void* out, int groups,
                             int64_t rows_per_group, int C, int relu, float drop_p,
                             uint64_t seed, const void* mask, void* keep_bits,
                             int x_dtype, int out_dtype, void* twin, int twin_dtype, mmh_stream_t s);

/* Backward of norm+relu+dropout.  dz = g * (relu||drop ? (out>0)/(1-p) : 1).
 * masked: 0 = no ReLU / dropout (`out` unused), 1 = `out` is the fp32 forward output,
 * 2 = `out` is the keep_bits array written by mmh_scale_shift_act.
 * reduce: s1[g][c] = sum dz, s2[g][c] = sum dz*xhat, xhat = (x-mean)*invstd.
 * apply:  dx = gamma*invstd*(dz - s1/count - xhat*s2/count).               */
size_t mmh_norm_bwd_ws_bytes(int groups, int64_t rows_per_group, int C);
int mmh_norm_bwd_reduce(const void* g, const void* out, const void* x,
                        const void* mean, const void* invstd, int groups,
                        int64_t rows_per_group, int C, int masked,
                        float drop_p, void* s1, void* s2, void* ws,
                        size_t ws_bytes, int g_dtype, int x_dtype, mmh_stream_t s);
int mmh_norm_bwd_apply(const void* g, const void* out, const void* x,
                       const void* mean, const void* invstd,
                       const void* gamma, const void* s1, const void* s2,
                       double count, int groups, int64_t rows_per_group,
                       int C, int masked, float drop_p, void* dx,
                       int g_dtype, int x_dtype, int dx_dtype, mmh_stream_t s);

/* The same backward in ONE pass for small planes (InstanceNorm at 64x64 and below; 16-bit x): a workgroup holds the whole
 * (group, 8-16 channels) plane in registers - g, x and the keep bits are read once, s1 / s2 summed on chip (and written
 * out: the affine parameters' gradients need them), dx applied.  Same per-element arithmetic as the two entry points
 * above, different (fixed) order of the plane sums.  Not for SyncBN (its sums cross ranks between the two passes).
 * mmh_norm_bwd_fused_supported: 1 when (groups, rows, C, masked, types) fit - rows <= 8192 / 8-channel lane groups.  */
int mmh_norm_bwd_fused_supported(int groups, int64_t rows, int C, int masked, int g_dtype, int x_dtype);
int mmh_norm_bwd_fused(const void* g, const void* out, const void* x, const void* mean, const void* invstd,
                       const void* gamma, double count, int groups, int64_t rows, int C, int masked, float drop_p,
                       void* s1, void* s2, void* dx, int g_dtype, int x_dtype, int dx_dtype, mmh_stream_t s);

/* ---- norm-apply fused into the consuming convolution (fp32, Winograd F(6x6,3x3) stack) ----
 * The reference runs conv -> Norm -> ReLU -> Dropout -> ReflectionPad -> conv as separate modules
 * (models/Generator.py:66-77, models/Discriminator.py:29-34).  Here the apply pass of the norm between
 * two 3x3 convs runs inside the second conv's input transform (mmh_wino_input_normact), and the apply
 * pass of its backward inside the first conv's backward transform (mmh_wino_input_dy_normbwd): the
 * activation between norm and conv, and the gradient between conv and norm, never reach HBM.  No
 * keep bits are stored either: the backward decides again from fma(x, scale, shift) > 0 - the
 * expression the forward evaluated - and the dropout bit array of the site.
 *
 * mmh_dropout_bits: bit e of byte i of `bits` [n/8] = element 8 i + e is kept (hash of (seed,
 * position) against p, or mask != NULL: uint8 per element, test hook).
 * *_rc: mmh_norm_bwd_reduce / _apply (fp32 tensors) with the keep decision taken again instead of
 * read; dbits NULL iff drop_p == 0.  C / 8 must be a power of two <= 256.                      */
int mmh_dropout_bits(int64_t n, float drop_p, uint64_t seed, const void* mask, void* bits,
                     mmh_stream_t s);
/* the same decisions as row words for the two transforms below, which walk one channel along image rows:
 * rows (uint32) [image_rows = B*H][ceil(W/32)][C], bit k of word j = element (row, 32 j + k, c)      */
int mmh_dropout_bits_rows(const void* bits, int64_t image_rows, int W, int C, void* rows,
                          mmh_stream_t s);
/* both arrays of an [image_rows][W][C] tensor in one launch (same decisions as the two calls above) */
int mmh_dropout_bits_both(int64_t image_rows, int W, int C, float drop_p, uint64_t seed,
                          const void* mask, void* bits, void* rows, mmh_stream_t s);
int mmh_norm_bwd_reduce_rc(const void* g, const void* x, const void* mean, const void* invstd,
                           const void* scale, const void* shift, const void* dbits, int groups,
                           int64_t rows_per_group, int C, int relu, float drop_p, void* s1,
                           void* s2, void* ws, size_t ws_bytes, mmh_stream_t s);
int mmh_norm_bwd_apply_rc(const void* g, const void* x, const void* mean, const void* invstd,
                          const void* gamma, const void* s1, const void* s2, const void* scale,
                          const void* shift, const void* dbits, double count, int groups,
                          int64_t rows_per_group, int C, int relu, float drop_p, void* dx,
                          mmh_stream_t s);
/* V = mmh_wino_input(dropout(relu(x*scale + shift)))   (tile 6, fp32; reflect 0 | 1; groups 1 | B;
 * drows = mmh_dropout_bits_rows, NULL iff drop_p == 0)                                           */
int mmh_wino_input_normact(const void* x, int B, int H, int W, int C, int reflect, void* V,
                           const void* scale, const void* shift, int groups, int relu,
                           float drop_p, const void* drows, mmh_stream_t s);
/* (V, Yh) = mmh_wino_input_dy(dx), dx = the result of mmh_norm_bwd_apply_rc(g, x, ...) computed per
 * element inside the transform (x = the norm's input = the forward output of the conv whose
 * backward this is).                                                                            */
int mmh_wino_input_dy_normbwd(const void* g, const void* x, int B, int H, int W, int C, void* V,
                              void* Yh, int fold, const void* mean, const void* invstd,
                              const void* gamma, const void* s1, const void* s2, double count,
                              const void* scale, const void* shift, const void* drows, int groups,
                              int relu, float drop_p, mmh_stream_t s);

/* dx = g * act'(y): relu -> (y>0), tanh -> 1-y^2 (Generator.py:259 head).   */
int mmh_act_bwd(const void* g, const void* y, void* dx, int64_t n, int act,
                mmh_stream_t s);
/* the same product written in 16 bits only (dtype MMH_BF16 | MMH_FP16; n % 8 == 0): the activation
 * backward of a conv whose dgrad is a 16-bit kernel and whose weights are frozen (VGG19 conv1_1 /
 * conv1_2 + ReLU, losses/L1_plus_perceptualLoss.py:22-27) - one pass instead of mmh_act_bwd +
 * mmh_cvt_lp16.                                                                               */
int mmh_act_bwd_lp16(const void* g, const void* y, int64_t n, int act, int dtype, void* out16,
                     mmh_stream_t s);
/* ... with g and / or y already in 16 bits (g_is16, y_is16; the storage type is `dtype`): the 16-bit edge between VGG19's
 * conv1_1 and conv1_2 (ops.VggPairFn) - the gradient comes out of conv1_2's 16-bit dgrad, the mask from conv1_1's 16-bit
 * output.                                                                                                      */
int mmh_act_bwd_lp16_io(const void* g, int g_is16, const void* y, int y_is16, int64_t n, int act, int dtype,
                        void* out16, mmh_stream_t s);

/* ---- PATBlock gate + concat (models/Generator.py:115-130) -----------------
 * out = x1 + s1*sigmoid(s2)*sigmoid(s3);  x2n = cat(s3,out); x3n = cat(s2,out)
 * x1,s1,s2,s3,out: [rows][C];  x2n,x3n: [rows][2C] (NULL -> not produced).
 * cat_dtype: element type of x2n / x3n, s23_dtype: of s2 / s3 (conv outputs)
 * (MMH_F32 | MMH_BF16 | MMH_FP16); x1, s1 and `out` are always fp32.        */
int mmh_patblock_gate_fwd(const void* x1, const void* s1, const void* s2,
                          const void* s3, void* out, void* x2n, void* x3n,
                          int64_t rows, int C, int cat_dtype, int s23_dtype, mmh_stream_t s);
/* g_out/g_x2n/g_x3n may be NULL (treated as zero).  gcat_dtype: element type of g_x2n / g_x3n
 * (gradients from 16-bit convolutions), s23_dtype: of s2 / s3, gs23_dtype: of g_s2 / g_s3. */
int mmh_patblock_gate_bwd(const void* g_out, const void* g_x2n,
                          const void* g_x3n, const void* s1, const void* s2,
                          const void* s3, void* g_x1, void* g_s1, void* g_s2,
                          void* g_s3, int64_t rows, int C, int gcat_dtype, int s23_dtype,
                          int gs23_dtype, mmh_stream_t s);

/* The gate with the block's LAST InstanceNorm inside (16-bit mode; models/Generator.py:66-77 + 115-130): s1 is not
 * materialised - the gate reads the stream-1 conv output y2 (16-bit, [groups * rows][C]) and scale / shift [groups][C] and
 * evaluates s1 = fma(y2, scale, shift) itself.  Backward: besides the gate's four gradients (g_s1 = the gradient of the
 * norm's output, fp32) the same launch leaves the norm backward's sums sum1[g][c] = sum g_s1, sum2[g][c] = sum g_s1 * xhat
 * (xhat = (y2 - mean) * invstd), taken in mmh_norm_bwd_reduce's chunks and order: follow it with mmh_norm_bwd_apply
 * (masked 0).  Bit-identical to mmh_scale_shift_act + mmh_patblock_gate_fwd and to mmh_patblock_gate_bwd +
 * mmh_norm_bwd_reduce.  ws: mmh_norm_bwd_ws_bytes(groups, rows, C).  x2n / x3n as in mmh_patblock_gate_fwd.   */
int mmh_patblock_gate_norm_supported(int groups, int64_t rows_per_group, int C);
int mmh_patblock_gate_norm_fwd(const void* x1, const void* y2, const void* scale, const void* shift,
                               const void* s2, const void* s3, void* out, void* x2n, void* x3n, int groups,
                               int64_t rows_per_group, int C, int y_dtype, int cat_dtype, int s23_dtype,
                               mmh_stream_t s);
int mmh_patblock_gate_norm_bwd(const void* g_out, const void* g_x2n, const void* g_x3n, const void* y2,
                               const void* scale, const void* shift, const void* mean, const void* invstd,
                               const void* s2, const void* s3, void* g_x1, void* g_s1, void* g_s2, void* g_s3,
                               void* sum1, void* sum2, void* ws, size_t ws_bytes, int groups,
                               int64_t rows_per_group, int C, int y_dtype, int gcat_dtype, int s23_dtype,
                               mmh_stream_t s);

/* ---- losses ----------------------------------------------------------------
 * GANLoss = BCEWithLogits vs a constant target, mean (network_utils.py:129-163)
 * L1 mean (L1_plus_perceptualLoss.py:37,66-67).  `out` is one device float:
 * out = weight * mean(...) with the mean taken over `denom` elements.       */
size_t mmh_reduce_ws_bytes(int64_t n);
int mmh_bce_logits_fwd(const void* x, int64_t n, float target, float weight,
                       double denom, void* out, void* ws, size_t ws_bytes,
                       mmh_stream_t s);
/* dx = gscalar[0] * weight/denom * (sigmoid(x) - target)                    */
int mmh_bce_logits_bwd(const void* x, int64_t n, float target, float weight,
                       double denom, const void* gscalar, void* dx,
                       mmh_stream_t s);
int mmh_l1_fwd(const void* a, const void* b, int64_t n, float weight,
               double denom, void* out, void* ws, size_t ws_bytes,
               mmh_stream_t s);
/* da = gscalar[0] * weight/denom * sign(a-b)                                */
int mmh_l1_bwd(const void* a, const void* b, int64_t n, float weight,
               double denom, const void* gscalar, void* da, mmh_stream_t s);
/* The perceptual term on 16-bit VGG features (losses/L1_plus_perceptualLoss.py:60-66 under apex O1, where the VGG
 * convolutions return fp16 and F.l1_loss runs on them): a16, b16 are the bf16 / fp16 feature maps (`dtype`), the
 * difference and the sum are fp32.  n % 8 == 0; ws as for mmh_l1_fwd (mmh_reduce_ws_bytes(n)).
 * mmh_l1_relu_bwd_lp16 is the L1 gradient folded with the mask of the ReLU that produced a16 (features[3]), written in
 * `dtype` for the 16-bit dgrad of conv1_2:  out16 = [a16 > 0] * gscalar[0] * weight/denom * sign(a16 - b16)          */
int mmh_l1_fwd_lp16(const void* a16, const void* b16, int64_t n, float weight,
                    double denom, int dtype, void* out, void* ws, size_t ws_bytes,
                    mmh_stream_t s);
int mmh_l1_relu_bwd_lp16(const void* a16, const void* b16, int64_t n, float weight,
                         double denom, const void* gscalar, int dtype, void* out16,
                         mmh_stream_t s);

/* MSE mean (F.mse_loss, the --percep_is_l1 0 branch of losses/L1_plus_perceptualLoss.py:68-71):
 * out = weight * sum (a-b)^2 / denom;  da = gscalar[0] * weight/denom * 2 (a-b)            */
int mmh_mse_fwd(const void* a, const void* b, int64_t n, float weight,
                double denom, void* out, void* ws, size_t ws_bytes,
                mmh_stream_t s);
int mmh_mse_bwd(const void* a, const void* b, int64_t n, float weight,
                double denom, const void* gscalar, void* da, mmh_stream_t s);

/* MaxPool2d(2, 2) of vgg19.features (indices 4, 9, 18, 27, 36) for --perceptual_layers > 3
 * (losses/L1_plus_perceptualLoss.py:22-27 slices the feature stack at any index).  NHWC fp32, even H and W, C % 4 == 0.
 * bwd: dx [B,H,W,C] receives g [B,H/2,W/2,C] at the first maximum of each window (scan order), zeros elsewhere.  */
int mmh_maxpool2x2_fwd(const void* x, int B, int H, int W, int C, void* y, mmh_stream_t s);
int mmh_maxpool2x2_bwd(const void* x, const void* g, int B, int H, int W, int C, void* dx, mmh_stream_t s);

/* ---- thin 7x7 convolutions (at most 4 output channels) on the vector ALU -----
 * The Generator head ReflectionPad2d(3)+Conv2d(64,3,7)+Tanh (models/Generator.py:255-259)
 * and the dgrad of the Discriminator stems (models/Discriminator.py:79-84) with respect
 * to the generated image only, i.e. the first <= 4 of their input channels
 * (MMHandModel.backward_G, models/MMHandModel.py:236-261: P2 / H1 carry no gradient).
 * A 32-wide MFMA tile wastes 7/8 of the matrix core on 4 columns; see conv_thin.hip.
 * fprop: d->Cout == 4, d->Cin % 4 == 0, 7x7 / stride 1 / pad 3 (reflect or zero), fp32;
 *        w [7][7][Cin][4]; same result as mmh_conv2d_fprop.
 * dgrad: writes channels [0,4) of dx (pixel stride d->x_cs) and leaves the others alone;
 *        w is the conv's full weight [7][7][d->Cin][d->Cout]; ws from the _ws_bytes query;
 *        dy_dtype: element type of dy (MMH_F32 | MMH_BF16 | MMH_FP16), arithmetic fp32. */
int mmh_conv7_thin_fprop(const mmh_conv_desc* d, const void* x, const void* w,
                         const void* bias, void* y, int act, mmh_stream_t s);
size_t mmh_conv7_thin_dgrad_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_thin_dgrad(const mmh_conv_desc* d, const void* dy, const void* w,
                         void* dx, void* ws, size_t ws_bytes, int dy_dtype, mmh_stream_t s);
/* wgrad of the head (d->Cout == 4, d->Cin % 64 == 0): dw [7][7][Cin][4] (+)= sum over pixels;
 * per-workgroup partial sums in ws, added in a fixed order (deterministic).              */
size_t mmh_conv7_thin_wgrad_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_thin_wgrad(const mmh_conv_desc* d, const void* x, const void* dy, void* dw,
                         void* ws, size_t ws_bytes, int accumulate, mmh_stream_t s);

/* The input gradient of the Generator head (ReflectionPad2d(3) + Conv2d(64, 3, 7): models/Generator.py:254-259, reached
 * from the L1 / perceptual / GAN losses of models/MMHandModel.py:236-275) in 16-bit mode, as a stem-shaped convolution
 * (conv_stem16.hip): dy fp32 [B,H,W,y_cs] (channels 0..3: the head's Cout padded to 4) is embedded, in 16 bits and 8
 * channels, into the zero-padded (H+6) x (W+6) domain, convolved 'same' with the mirrored, transposed filter (4 -> 64
 * channels) and the pad ring folded back (the transpose of ReflectionPad2d(3)): dx fp32 or 16-bit [B,H,W,x_cs] (64
 * channels written).  d describes the head conv itself (Cin = 64, Cout = 4, 7x7, stride 1, MMH_PAD_REFLECT, 16-bit
 * dtype); w is its fp32 weight [7][7][64][4]; ws >= mmh_conv7_head_dgrad_lp16_ws_bytes(d), 256-byte aligned.          */
int mmh_conv7_head_dgrad_lp16_supported(const mmh_conv_desc* d);
size_t mmh_conv7_head_dgrad_lp16_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_head_dgrad_lp16(const mmh_conv_desc* d, const void* dy, const void* w, void* dx, int dx_is16, void* ws,
                              size_t ws_bytes, const void* zeros, mmh_stream_t s);

/* The same two convolutions from 16-bit tensors on the 16-column MFMA (conv7_n4.hip): an (8+6) x (16+6) pixel halo of
 * the 64-channel input and the whole [49][4][64] filter resident in LDS, 4 of the 16 weight rows meaningful.
 * mode 0: fprop of the Generator head (models/Generator.py:254-259): x16 [B,H,W,x_cs >= 64] 16-bit, w the head's fp32
 *         weight [7][7][64][Cout <= 4], y fp32 [B,H,W,y_cs] (channels 0..3 written), +bias, activation.
 * mode 1: gradient of a Discriminator stem towards its first four input channels (models/Discriminator.py:60-64 from
 *         models/MMHandModel.py:238-243): x16 = dy16 [B,H,W,y_cs >= 64], w the stem's fp32 weight [7][7][Cin][64],
 *         y = dx fp32 [B,H,W,x_cs]: channels [0,4) written, the others left alone (as mmh_conv7_thin_dgrad).  With
 *         MMH_PAD_REFLECT the kernel runs over the padded domain into ws and the pad ring is folded back.
 *         Also 3x3 / pad 1 / zero padding with Cin == 4: VGG19 conv1_1 seen from the perceptual loss
 *         (losses/L1_plus_perceptualLoss.py:22-27,60-67).
 * ws (mmh_conv7_n4_lp16_ws_bytes): the 16-bit filter twin, built by the call, + the padded-domain gradient.        */
int mmh_conv7_n4_lp16_supported(const mmh_conv_desc* d, int mode);
size_t mmh_conv7_n4_lp16_ws_bytes(const mmh_conv_desc* d, int mode);
int mmh_conv7_n4_lp16(const mmh_conv_desc* d, int mode, const void* x16, const void* w,
                      const void* bias, void* y, int act, void* ws, size_t ws_bytes,
                      const void* zeros, mmh_stream_t s);

/* wgrad of the 7x7 / stride 1 / ReflectionPad2d(3) stems (models/Generator.py:158-168,
 * models/Discriminator.py:60-64; fp32, Cin 8 | 44 (where it beats the generic kernel), Cout == 64 dense, H % 2 == 0,
 * W % 64 == 0): the input is reflect-padded once into ws, a workgroup stages the two input rows of a
 * filter row and a 2 x 64 pixel tile in LDS and both MFMA operands are plain LDS reads - every input
 * element is read 7 times instead of 49.  dw [7][7][Cin][64] (+)= ...; split-K slabs in ws, summed in a
 * fixed order.                                                                              */
int mmh_conv7_stem_wgrad_supported(const mmh_conv_desc* d);
size_t mmh_conv7_stem_wgrad_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_stem_wgrad(const mmh_conv_desc* d, const void* x, const void* dy, void* dw,
                         void* ws, size_t ws_bytes, int accumulate, mmh_stream_t s);

/* ---- compacted-channel fp32 7x7 stems for inputs that are mostly pose heat maps (stem_sparse.hip) -----
 * The Generator's pose stem and D_PB (models/Generator.py:158-164, models/Discriminator.py:60-64) read 21 / 42 truncated
 * Gaussians (about 1.6 % of a 256 x 256 map is non-zero); these kernels contract over the channels that are active in a tile.
 *
 * mmh_stem_activity: x fp32 NHWC [B,H,W,C] dense (4 <= C <= 48, C % 4 == 0, H % 8 == 0, W % 16 == 0, 16-byte aligned) ->
 *   mask uint64 [B][H/8][W/16] (mmh_stem_activity_bytes; 0 for an unsupported shape): bit c is set iff channel c has an
 *   element != 0 (-0.0 counts as zero, NaN as non-zero) inside the block's 8 x 16 pixels plus the 3-pixel halo, read through
 *   the ReflectionPad2d(3) index map.  Exact; one pass; every block writes its own word.
 * mmh_conv7_stem_sparse_fprop: what mmh_conv2d_fprop_stats writes for the same stem (y and the whole stats buffer, stats may
 *   be NULL), bit for bit, for finite weights (an omitted term is fmaf(0, w, acc); with a non-finite w the dense kernel gives
 *   NaN where this one gives a number).  `mask` must be mmh_stem_activity of this x.  Not under "conv_levels" 2.
 * mmh_conv7_stem_sparse_wgrad (W % 64 == 0): dw [7][7][Cin][64] fp32 (+)= the stem's weight gradient; a workgroup per (input
 *   channel, split) walks mmh_conv7_stem_wgrad's 2 x 64 pixel tiles of that split in its order and multiplies only those
 *   whose mask words have the channel; slabs [splits][7][7][Cin][64] in ws (16-byte aligned) summed as that kernel's are.
 *   Where mmh_conv7_stem_wgrad_supported(d), dw is that kernel's bit for bit (finite dy); elsewhere (24 lanes) it is the
 *   same sum in another order than mmh_conv2d_wgrad's - callers that need the parent's bits keep the dense route there.
 * Results never depend on the sparsity; a fully dense input is only slower.  "stem_sparse" 0 turns both _supported off.  */
size_t mmh_stem_activity_bytes(int B, int H, int W);
int mmh_stem_activity(const void* x, int B, int H, int W, int C, void* mask, mmh_stream_t s);
int mmh_conv7_stem_sparse_fprop_supported(const mmh_conv_desc* d);
int mmh_conv7_stem_sparse_fprop(const mmh_conv_desc* d, const void* x, const void* mask, const void* w, const void* bias,
                                void* y, void* stats, mmh_stream_t s);
int mmh_conv7_stem_sparse_wgrad_supported(const mmh_conv_desc* d);
size_t mmh_conv7_stem_sparse_wgrad_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_stem_sparse_wgrad(const mmh_conv_desc* d, const void* x, const void* mask, const void* dy, void* dw, void* ws,
                                size_t ws_bytes, int accumulate, mmh_stream_t s);
/* mmh_conv7_stem_sparse_wgrad_flat (W % 16 == 0, B H W < 2^25, x 16-byte aligned, x_cs % 4 == 0): the same gradient in the
 *   order of mmh_conv2d_wgrad's generic kernel, the dense route of the stems mmh_conv7_stem_wgrad does not take (D_PB, 24
 *   lanes): its splits and pixels per split (one shared rule: option "wgrad_slots" moves both), its 32-pixel k-steps and
 *   k-slot pairs, its slab sum.  A workgroup per (group of four adjacent lanes, split) multiplies a step only for the
 *   lanes whose bit one of the step's two mask words has; always-active lanes share their group's pass over dy.  dw is
 *   mmh_conv2d_wgrad's bit for bit (finite dy, up to the sign of an exact zero); ws_bytes equals
 *   mmh_conv2d_wgrad_ws_bytes(d).  _supported is 0 under "stem_sparse" 0 or "stem_sparse_flat" 0 (default 1).          */
int mmh_conv7_stem_sparse_wgrad_flat_supported(const mmh_conv_desc* d);
size_t mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(const mmh_conv_desc* d);
int mmh_conv7_stem_sparse_wgrad_flat(const mmh_conv_desc* d, const void* x, const void* mask, const void* dy, void* dw, void* ws,
                                     size_t ws_bytes, int accumulate, mmh_stream_t s);

/* ---- Adam (torch.optim.Adam, MMHandModel.py:90-98) over a flat buffer ------
 * step is the 1-based step count; no weight decay, no amsgrad.
 * skip_flag (device int32, may be NULL): when *skip_flag != 0 the launch leaves
 * p, m and v untouched - the `if not self.overflow: optimizer.step()` of
 * MMHandModel.py:316-328 decided on the device, without a host round trip.
 * loss_scale (device float, may be NULL): the gradient is additionally divided by
 * *loss_scale - the unscale step of dynamic loss scaling, read on the device.  */
int mmh_adam_step(void* p, const void* g, void* m, void* v, int64_t n,
                  float lr, float beta1, float beta2, float eps, int step,
                  float grad_scale, const void* skip_flag, const void* loss_scale,
                  mmh_stream_t s);

/* The same update with the step count and the learning rate resident on the device - nothing in the launch depends on the
 * iteration, so a whole training step can sit in a captured hipGraph (MMHandModel.py:310-330 replayed).  step (device
 * int32): incremented first, unless *skip_flag != 0 (apex does not count a skipped step: no host correction afterwards);
 * lr (device float): what update_learning_rate (models/base_model.py:82-87) last wrote; coef (device float[2]): scratch
 * for lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t), computed in double as mmh_adam_step does on the host.             */
int mmh_adam_step_dev(void* p, const void* g, void* m, void* v, int64_t n, const void* lr, float beta1, float beta2,
                      float eps, void* step, float grad_scale, const void* skip_flag, const void* loss_scale, void* coef,
                      mmh_stream_t s);

/* Dropout in a captured step: every kernel that draws dropout decisions from a by-value seed (mmh_scale_shift_act[_twin],
 * mmh_dropout_bits[_both]) adds *salt (a device uint64; NULL = none, the default) to that seed when it RUNS.  The salt is
 * read from the pointer registered here at launch time; mmh_u64_add advances it on the stream (inside the graph), so each
 * replay of the same launches draws fresh masks (models/Generator.py:66-77 nn.Dropout(0.5) per forward).              */
int mmh_set_dropout_salt(const void* salt_u64);
int mmh_u64_add(void* value_u64, uint64_t inc, mmh_stream_t s);

/* ImagePool.query (util/image_pool.py:14-34) on a device-resident pool [slots][elems_per_image] fp32 with the host's
 * decisions as device int32 indices [B]: out[i] = src_idx[i] >= 0 ? pool[src_idx[i]] (content before this query)
 * : images[-1 - src_idx[i]]; then pool[dst_idx[i]] = images[i] where dst_idx[i] >= 0 (the host emits one writer per slot).
 * The launches are the same every iteration - only the index arrays change - so the query can sit in a captured step.  */
int mmh_pool_exchange(void* pool, const void* images, void* out, const void* src_idx, const void* dst_idx, int B,
                      int64_t elems_per_image, mmh_stream_t s);

/* ---- overflow detection (MMHandModel.loss_backward, MMHandModel.py:294-308) --
 * *flag_out = (flag_in ? *flag_in : 0) | any(!isfinite(g[0..n))).  flag_in carries
 * the sticky `self.overflow` of the steps already taken this iteration.  Run on
 * the flat gradient buffer AFTER the data-parallel all-reduce: a non-finite
 * value on any rank is non-finite in the sum on every rank, which is the
 * flag all-reduce of reduce_tensor (MMHandModel.py:381-384) for free.
 * own_out (device int32, may be NULL) = any(!isfinite(g)) of THIS gradient alone: what
 * apex's per-loss scaler sees when its scale_loss context exits.               */
int mmh_grad_nonfinite(const void* g, int64_t n, const void* flag_in,
                       void* flag_out, void* own_out, mmh_stream_t s);

/* ---- dynamic loss scaling (apex.amp.initialize(..., num_losses=3) + amp.scale_loss,
 * MMHandModel.py:99-108,294-299): state = {scale, clean steps} (2 device floats).  The
 * backward runs on loss * scale; mmh_adam_step(loss_scale = state) divides it out again;
 * then, as apex's LossScaler.update_scale: *overflow != 0 -> scale = max(scale * backoff,
 * min_scale), clean = 0; else ++clean, and clean == interval -> scale = min(scale * growth,
 * max_scale), clean = 0.  apex's dynamic defaults: start 2^16, growth 2, backoff 0.5,
 * interval 2000, max 2^24.                                                           */
int mmh_loss_scale_update(void* state, const void* overflow, float growth, float backoff,
                          int interval, float min_scale, float max_scale, mmh_stream_t s);

/* ---- layout: NCHW (any strides) <-> padded NHWC, with channel concat -------
 * replaces torch.cat at MMHandModel.py:216-220,238,242,278-289.            */
typedef struct mmh_plane_src {
    void* ptr;                       /* NULL -> skipped                     */
    int32_t C;                       /* channels taken from this source     */
    int64_t sb, sc, sh, sw;          /* element strides                     */
} mmh_plane_src;
/* Cd % 4 == 0, nhwc 16-byte aligned.
 * dir 0: gather srcs -> nhwc[B,H,W,Cd] (channels beyond sum(C) zeroed).
 * dir 1: scatter nhwc -> srcs (backward of dir 0 / NHWC->NCHW export).     */
int mmh_pack_nhwc(const mmh_plane_src* srcs, int nsrc, void* nhwc, int B,
                  int H, int W, int Cd, int dir, mmh_stream_t s);
/* The gather (dir 0) staged through LDS - 256 pixels per workgroup, read with the lanes along the pixels of a source
 * plane, written as whole 16-byte lanes in address order - with, in the same pass, the 16-bit copy out16 [B,H,W,C8]
 * (channels zero-padded to C8, C8 % 8 == 0, Cd <= C8 <= 56; dtype MMH_BF16 | MMH_FP16) that the 16-bit 7x7 stems read:
 * what mmh_lp16_pad_cvt would make of nhwc, bit for bit.  nhwc or out16 may be NULL (only the other one is written).
 * Cd % 4 == 0, Cd <= 56 (58 KB of LDS).  (MMHandModel.py:216-220,238,242,278-289: the concatenations in front of every stem.)      */
int mmh_pack_nhwc_lp16(const mmh_plane_src* srcs, int nsrc, void* nhwc, void* out16, int B, int H, int W,
                       int Cd, int C8, int dtype, mmh_stream_t s);

/* ---- pose maps (data/generic_dataset.py:191-217,239-242; util/util.py:94-114)
 * uv: [n_maps][2] float64 (x,y).  out: [n_maps][H][W] fp32 =
 * clamp/threshold(exp(-((gx-x)^2+(gy-y)^2)/(2 sigma^2))) computed in f64.  */
int mmh_pose_heatmaps(const void* uv, int n_maps, int H, int W, double sigma,
                      void* out, mmh_stream_t s);
/* cords[n_maps][2] int32 = (y,x) of the first (row-major) arg-max above
 * `threshold`, or (-1,-1).  maps: [n_maps][H][W] fp32.                      */
int mmh_map_to_cord(const void* maps, int n_maps, int H, int W,
                    float threshold, void* cords, mmh_stream_t s);

/* ---- on-device input pipeline (data/generic_dataset.py:133-180) ---------------
 * One kernel turns what the loader workers produce per sample on the CPU —
 * normalize(BGR->RGB image), 21 pose maps per hand, depth = 256*G+R -> /700 ->
 * (.-0.5)/0.5 replicated x3 — into the stems' NHWC buffers directly:
 *   img1,img2 : uint8 [B,H,W,3] BGR (as cv2.imread returns them)
 *   dep1,dep2 : uint8 [B,H,W,3] BGR depth PNGs
 *   uv1,uv2   : float64 [B,21,2] joint (x,y)
 *   x_h1,x_h2 : fp32 [B,H,W,4]  RGB in [-1,1], lane 3 = 0
 *   x_p       : fp32 [B,H,W,44] P1 in 0..20, P2 in 21..41, lanes 42,43 = 0
 *   x_d       : fp32 [B,H,W,8]  D1 x3, D2 x3, lanes 6,7 = 0
 * All arithmetic is float64 then cast, exactly as numpy does it in the reference. */
int mmh_decode_inputs(const void* img1, const void* img2, const void* dep1,
                      const void* dep2, const void* uv1, const void* uv2,
                      int B, int H, int W, double sigma, void* x_h1, void* x_h2,
                      void* x_p, void* x_d, mmh_stream_t s);
/* The same pass with the resize inside it: sources uint8 [B,Hs,Ws,3] BGR at the files'
 * size, the four outputs (layouts as above) at Ho x Wo.  Bilinear with half-pixel centres
 * and edge clamp, per output pixel: sx = (x + 0.5) * Ws / Wo - 0.5 clamped below at 0,
 * x0 = floor(sx), x1 = min(x0 + 1, Ws - 1), weight sx - x0, the same in y - what
 * F.interpolate(mode="bilinear", align_corners=False, antialias=False) samples; it up- and
 * down-scales, with independent ratios in H and W.  The four taps are combined in float64
 * from the raw bytes (colour per channel, depth as 256*G + R per tap), the result goes
 * through the normalisation above in float64, and the store is the only rounding.
 * uv1, uv2 are joints ALREADY scaled to the output grid, u' = (u + 0.5) * Wo / Ws - 0.5,
 * v' = (v + 0.5) * Ho / Hs - 0.5: the pose maps are the Gaussians of mmh_decode_inputs on
 * output pixel coordinates (sigma is not scaled).  The outputs must be 16-byte aligned.  */
int mmh_decode_inputs_resized(const void* img1, const void* img2, const void* dep1,
                              const void* dep2, const void* uv1, const void* uv2,
                              int B, int Hs, int Ws, int Ho, int Wo, double sigma,
                              void* x_h1, void* x_h2, void* x_p, void* x_d, mmh_stream_t s);

/* ---- resident dataset: the decoded images stay in device memory, batches are named by slot ----
 * replaces the loop of data/mmhand_dataset_data_loader.py:22-48 over data/generic_dataset.py:133-180
 * that re-reads and re-decodes every file every epoch (fixed order, no shuffle, a sampler whose
 * epoch never advances: every epoch asks for the same files).
 * mmh_store_images scatters a decoded batch into the store:
 *   src    uint8 [N,H,W,3]
 *   slots  device int32 [N]: image n goes to store[slots[n]]; -1 = skip this image
 *   store  uint8 [S,H,W,3]
 *   status device int32 [1] or NULL: a slot outside [-1, S) writes nothing and ORs 1 into it */
int mmh_store_images(const void* src, const void* slots, int N, int H, int W,
                     void* store, int64_t S, void* status, mmh_stream_t s);
/* mmh_decode_inputs / mmh_decode_inputs_resized reading their sources out of a resident store
 * instead of a batch (data/generic_dataset.py:133-180 without its cv2.imread calls, and with
 * data/mmhand_dataset_data_loader.py:22-48's collation reduced to a row of slots):
 *   store    uint8 [S,Hs,Ws,3] BGR
 *   idx      device int32 [B,4] = slots of (img1, img2, dep1, dep2) of each sample
 *   uv_table float64 [S,21,2], joints ALREADY on the Ho x Wo grid; sample b takes rows
 *            idx[b][0] and idx[b][1]
 * Outputs and arithmetic are exactly those two entry points' (Ho x Wo == Hs x Ws is the plain
 * pass); the outputs must be 16-byte aligned.  A sample with a slot outside [0, S) is written as
 * zeros (all of its lanes) and ORs 1 into *status (device int32 [1], may be NULL); every byte
 * offset into the store is 64-bit.                                                          */
int mmh_decode_inputs_indexed(const void* store, int64_t S, int Hs, int Ws, const void* idx,
                              const void* uv_table, int B, int Ho, int Wo, double sigma,
                              void* x_h1, void* x_h2, void* x_p, void* x_d, void* status,
                              mmh_stream_t s);

/* ---- geometric augmentation inside the decode pass (--augment_geom) ----------------------
 * an addition: the reference declares --no_flip / --use_flip (options/base_options.py) and
 * never reads them; its loader (data/generic_dataset.py:133-180) has no spatial augmentation.
 * mmh_decode_inputs_resized sampling through one inverse affine map per image and side:
 *   xf  float64 [B,2,6], row-major [a00 a01 a02; a10 a11 a12] per (sample, side); side 0
 *       samples img1 and dep1, side 1 samples img2 and dep2
 * The output pixel (x, y) of the Ho x Wo grid reads the source coordinate
 *   sx = (a00*x + a01*y) + a02,  sy = (a10*x + a11*y) + a12
 * in float64, each product and sum rounded on its own (no fused multiply-add), clamped to
 * [0, Ws-1] x [0, Hs-1] before any conversion to an integer (edge replicate; a NaN lands on
 * 0, no matrix can index outside the image); x0 = min(floor(sx), Ws-1), x1 = min(x0+1, Ws-1),
 * weight sx - x0, the same in y.  This is F.grid_sample(mode="bilinear",
 * padding_mode="border", align_corners=True) on pixel coordinates.  Taps, normalisation,
 * layouts and alignment as mmh_decode_inputs_resized; uv1, uv2 are joints ALREADY transformed
 * onto the output grid (sigma is not scaled).                                                */
int mmh_decode_inputs_affine(const void* img1, const void* img2, const void* dep1,
                             const void* dep2, const void* uv1, const void* uv2,
                             const void* xf, int B, int Hs, int Ws, int Ho, int Wo,
                             double sigma, void* x_h1, void* x_h2, void* x_p, void* x_d,
                             mmh_stream_t s);
/* The same reading its sources out of a resident store, as mmh_decode_inputs_indexed does:
 *   uv  float64 [B,2,21,2] per SAMPLE (side 0, side 1), already on the output grid - not the
 *       per-slot table, the joints change with every epoch's transform
 *   xf  float64 [B,2,6] as above
 * Slot guards, status and 64-bit store offsets are mmh_decode_inputs_indexed's.             */
int mmh_decode_inputs_indexed_affine(const void* store, int64_t S, int Hs, int Ws,
                                     const void* idx, const void* uv, const void* xf, int B,
                                     int Ho, int Wo, double sigma, void* x_h1, void* x_h2,
                                     void* x_p, void* x_d, void* status, mmh_stream_t s);

/* ---- data-parallel gradient all-reduce (apex DistributedDataParallel behind
 * models/MMHandModel.py:109-116; reduce_tensor :381-384) -------------------------
 * The training process already holds ONE RCCL communicator per GPU (torch.distributed's "nccl"
 * backend is RCCL on ROCm).  mmh_rccl_bind resolves ncclAllReduce from the RCCL image that
 * communicator lives in (the path of the librccl the process has loaded; no link-time
 * dependency, no second RCCL).  mmh_allreduce_bucket enqueues the in-place SUM all-reduce of
 * `count` elements of type `dtype` (MMH_F32 | MMH_BF16 | MMH_FP16) at `buf` - a contiguous
 * bucket of a network's flat gradient buffer - on communicator `comm` (an ncclComm_t) and
 * stream `s`; the 1/world factor is folded into mmh_adam_step.  Every rank must issue its
 * buckets in the same order (mmhand_amd/dp.py cuts them in reverse layer order).
 * mmh_rccl_comm_ranks: the communicator's rank count, -1 if unbound / invalid.              */
int mmh_rccl_bind(const char* librccl_path);
int mmh_rccl_comm_ranks(void* comm);
int mmh_allreduce_bucket(void* comm, void* buf, int64_t count, int dtype, mmh_stream_t s);

/* ---- image quality metrics (pytorch_ssim/__init__.py:17-37, baselines/quantitative_on_benchmarks/utils.py:100-111) ----
 * replaces ssim(pred, gt) of the Evaluator, one image at a time, plus mean |a-b| and mean (a-b)^2 from the same pass.
 * Every image pair is [C][H][W] and mapped to [0, 1] on load: v = stored * scale + offset (generator output in [-1, 1]:
 * 0.5 / 0.5; 8-bit pixels: 1/255 / 0).  taps (host memory, `window` floats, window odd, 3 .. 15): the 1-D window as
 * pytorch_ssim.gaussian(window, 1.5) returns it (fp32, normalised by torch's fp32 sum - its last bit is torch's summation
 * order, which is why the caller passes it); the 2-D window is their fp32 outer product; zero padding of window / 2;
 * ssim_map = ((2 mu_a mu_b + c1)(2 s_ab + c2)) / ((mu_a^2 + mu_b^2 + c1)(s_a^2 + s_b^2 + c2)) (c1 = 0.01^2, c2 = 0.03^2
 * in the reference).  out[b][0] = mean of ssim_map over C, H, W (the reference's size_average=False), out[b][1] =
 * mean |a-b|, out[b][2] = mean (a-b)^2, float64.  Within 1e-6 of the same formula in float64 (fp32 moments, each
 * taken about a pixel inside its own window); no atomics: an image's result is bit-identical run to run and does not
 * depend on the other images of the batch; ssim(a, b) == ssim(b, a) bit for bit and ssim(x, x) == 1.
 * ws: mmh_image_metrics_ws_bytes(B, C, H, W, window) bytes (0 = the arguments are refused).                             */
enum { MMH_U8 = 3 };             /* mmh_image_src only: uint8 pixels                                                    */
typedef struct mmh_image_src {
    const void* ptr;                 /* element (b, c, h, w) at ptr + b sb + c sc + h sh + w sw (elements)              */
    int32_t dtype;                   /* MMH_F32 | MMH_BF16 | MMH_FP16 | MMH_U8                                          */
    float scale, offset;             /* [0, 1] value = stored * scale + offset                                          */
    int64_t sb, sc, sh, sw;          /* element strides; negative allowed (BGR pixels read as RGB: sc = -1)             */
} mmh_image_src;
size_t mmh_image_metrics_ws_bytes(int B, int C, int H, int W, int window);
int mmh_image_metrics(const mmh_image_src* a, const mmh_image_src* b, int B, int C, int H, int W, int window, const float* taps,
                      double c1, double c2, void* ws, size_t ws_bytes, double* out /* [B][3]: ssim, l1, mse */,
                      mmh_stream_t s);

/* ---- the same pass with a region mask (evaluate --hand_region): mmh_image_metrics plus the three means over a mask's pixels ----
 * a, b, B .. c2 as mmh_image_metrics (window 3 .. 15, caller-passed fp32 taps, the four storage types, any strides).
 * mask: uint8 [B][H][W], element (b, y, x) at mask + b msb + y msh + x msw (bytes); non-zero = inside; one mask serves all C
 * channels of its image.  One pass writes, float64,
 *   out[b][0..2] = ssim, l1, mse of the whole image, bit-identical to mmh_image_metrics on the same inputs;
 *   out[b][3..5] = the same zero-padded ssim_map (computed from the unmasked images), |a-b| and (a-b)^2 averaged over the mask's
 *                  pixels and the C channels: sum * (1.0 / ((double)C * count)), the float64 sums taken in the same fixed order as
 *                  the whole-image sums (a pixel outside the mask contributes 0.0 in its place), so an all-ones mask returns the
 *                  whole-image bits; NaN where count = 0;
 *   out[b][6]    = count, the number of non-zero mask bytes of image b.
 * No atomics: an image's result is bit-identical run to run and does not depend on the batch; f(a, b) == f(b, a) bit for bit.
 * ws: mmh_image_metrics_masked_ws_bytes(B, C, H, W, window) bytes (0 = the arguments are refused).                            */
size_t mmh_image_metrics_masked_ws_bytes(int B, int C, int H, int W, int window);
int mmh_image_metrics_masked(const mmh_image_src* a, const mmh_image_src* b, const uint8_t* mask, int64_t msb, int64_t msh,
                             int64_t msw, int B, int C, int H, int W, int window, const float* taps, double c1, double c2, void* ws,
                             size_t ws_bytes, double* out /* [B][7] */, mmh_stream_t s);

/* ---- multi-scale SSIM (Wang, Simoncelli, Bovik 2003) from the same tile pass (evaluate --ms_ssim) -------------------------------
 * a, b, B .. c2 as mmh_image_metrics.  levels L in 1 .. 5; weights: host memory, L doubles, each finite and > 0.
 * Level 0 is the pair mapped to [0, 1]; level l + 1 is level l averaged 2 x 2 in fp32: pooled pixel (i, j) =
 * ((v00 + v01) + (v10 + v11)) * 0.25f, evaluated as written, over rows 2 i - ph, 2 i - ph + 1 and columns 2 j - pw, 2 j - pw + 1
 * with ph = H_l % 2, pw = W_l % 2; values outside the image are zero and the divisor is always 4 - torch's
 * F.avg_pool2d(x, 2, padding=(H % 2, W % 2)); H_{l+1} = (H_l + 1) / 2 (integer division), likewise W.  The workgroup that scores
 * a tile of level l writes its part of level l + 1 from the halo it holds (the pyramid lies in the workspace; no separate pooling
 * pass reads a level).
 * At level l only the output pixels whose whole window lies inside the image count: window / 2 <= y < H_l - window / 2, likewise
 * x - count_l = (H_l - window + 1)(W_l - window + 1) - where the zero-padded ssim_map of mmh_image_metrics equals a "valid"
 * convolution.  With s_a^2, s_b^2, s_ab of that map, cs = (2 s_ab + c2) / ((s_a^2 + s_b^2) + c2), written like the ssim
 * expression without contraction in mirror-image form: cs(x, x) == 1 and cs(a, b) == cs(b, a) bitwise.
 * Per image b and channel c, v_l = (fixed-order float64 sum over the counted pixels) * (1.0 / count_l) of cs for l < L - 1 and of
 * ssim_map for l = L - 1;  scales[b][c][l] = v_l (unclamped);  out[b] = (sum over c of prod over l of pow(max(v_l, 0),
 * weights[l])) / C, float64.  Each v_l is within 1e-6 of the float64 formula on the fp32-pooled level.  No atomics: bit-identical
 * run to run, independent of the batch, symmetric in (a, b) bit for bit, 1.0 for a == b.
 * Refused (ws_bytes 0, non-zero return before any launch): the shape limits of mmh_image_metrics, levels outside 1 .. 5, and
 * min(H, W) <= (window - 1) * 2^(L - 1) (at L = 5 and window 11: min side > 160; the last level then holds a whole window).
 * ws: mmh_ms_ssim_ws_bytes(B, C, H, W, window, levels) bytes, 8-byte aligned.                                                  */
size_t mmh_ms_ssim_ws_bytes(int B, int C, int H, int W, int window, int levels);
int mmh_ms_ssim(const mmh_image_src* a, const mmh_image_src* b, int B, int C, int H, int W, int window, const float* taps, double c1,
                double c2, int levels, const double* weights, void* ws, size_t ws_bytes, double* scales /* [B][C][levels] */,
                double* out /* [B] */, mmh_stream_t s);

/* ---- PNG decode of a batch on the device (data/generic_dataset.py:140-149: the four cv2.imread calls per sample) ----------
 * N zlib streams - each the concatenated IDAT payload of ONE 8-bit, colour type 2 (RGB), non-interlaced PNG of H x W pixels,
 * which is what cv2.imwrite and PIL write for the prepared RHD / STB directories - are inflated (RFC 1950 / 1951: stored, fixed
 * and dynamic blocks), checked against their Adler-32 trailer, unfiltered (PNG filter types 0 - 4) and written as the pixels
 * cv2.imread returns, in one launch, one wave per image.
 *   streams : device bytes, streams_bytes of them; image i's stream is [offsets[i], offsets[i + 1])
 *   offsets : device int64 [N + 1], non-decreasing, inside [0, streams_bytes] (an image whose range is not gets
 *             MMH_PNG_E_RANGE; nothing outside a valid range is ever read)
 *   scratch : device bytes, N * H * (1 + 3 W): the filtered scanlines of every image
 *   out     : device uint8 [N][H][W][3], B,G,R per pixel if bgr != 0 (cv2.imread's order), else R,G,B
 *   status  : device int32 [N]: MMH_PNG_OK or the first error of that image (the enum below).  An image with a non-zero status
 *             leaves its out slot undefined and does not disturb the other images of the launch.
 * Host-side argument errors (N < 0, H or W < 1, H * (1 + 3 W) >= 2^31, a null pointer with N > 0) return non-zero before any
 * launch.  The container (signature, IHDR, chunk CRCs) is the host's: mmhand_amd/png.py.                                     */
enum {
    MMH_PNG_OK = 0,
    MMH_PNG_E_HEADER = 1,           /* zlib header: CM != 8, window > 32 KiB or FCHECK                                   */
    MMH_PNG_E_DICT = 2,             /* preset dictionary flag                                                            */
    MMH_PNG_E_TRUNCATED = 3,        /* the stream ends inside a block or the trailer                                     */
    MMH_PNG_E_BLOCK_TYPE = 4,       /* reserved block type 3                                                             */
    MMH_PNG_E_STORED_LEN = 5,       /* stored block: LEN != ~NLEN                                                        */
    MMH_PNG_E_CODE_OVER = 6,        /* over-subscribed code lengths                                                      */
    MMH_PNG_E_CODE_INCOMPLETE = 7,  /* incomplete code lengths (other than one single 1-bit code)                        */
    MMH_PNG_E_REPEAT = 8,           /* code-length symbol 16 with no previous length                                     */
    MMH_PNG_E_CODE_COUNT = 9,       /* more than 286 / 30 codes announced, or a repeat runs past them                    */
    MMH_PNG_E_NO_EOB = 10,          /* no code for end-of-block                                                          */
    MMH_PNG_E_SYMBOL = 11,          /* length symbol 286 / 287 or distance symbol 30 / 31                                */
    MMH_PNG_E_BAD_CODE = 12,        /* a bit pattern no code of an (accepted) incomplete set has                         */
    MMH_PNG_E_DISTANCE = 13,        /* a match reaches before the start of the output                                    */
    MMH_PNG_E_OUTPUT_LONG = 14,     /* more than H * (1 + 3 W) bytes                                                     */
    MMH_PNG_E_OUTPUT_SHORT = 15,    /* the final block ends with fewer                                                   */
    MMH_PNG_E_TRAILING = 16,        /* bytes after the Adler-32 trailer                                                  */
    MMH_PNG_E_ADLER = 17,           /* Adler-32 mismatch                                                                 */
    MMH_PNG_E_FILTER = 18,          /* a scanline's filter byte is above 4                                               */
    MMH_PNG_E_STEPS = 19,           /* the step bound of the decoder tripped (cannot happen: every step consumes input)  */
    MMH_PNG_E_RANGE = 20            /* offsets[i] .. offsets[i + 1] is not a range of the stream buffer                  */
};
int mmh_png_decode_batch(const void* streams, int64_t streams_bytes, const int64_t* offsets, int N, int H, int W, void* scratch,
                         void* out, int32_t* status, int bgr, mmh_stream_t s);

/* ---- PNG encode of a batch on the device (aug.py:66-71: one cv2.imwrite per generated image) ---------------------------------
 * N images of H x W 8-bit pixels -> N zlib streams, each the whole IDAT payload of an 8-bit, colour type 2, non-interlaced
 * PNG: every row filtered with the type (0 - 4) of the smallest sum of absolute values, then Huffman-only DEFLATE - one
 * dynamic block of literals per 16 rows, no matches - and the Adler-32 trailer.  Two launches over (image, 16-row segment).
 *   pixels     : device uint8 [N][H][W][3], B,G,R per pixel if bgr != 0, else R,G,B (the stream always holds R,G,B)
 *   scratch    : device bytes, mmh_png_encode_scratch_bytes(N, H, W) of them, 16-byte aligned
 *   streams    : device bytes, N slots of slot_bytes each; image i's stream is the first lengths[i] bytes of slot i, the rest
 *                of the slot is left as it was
 *   lengths    : device int64 [N]
 *   status     : device int32 [N]: MMH_PNGENC_OK, or MMH_PNGENC_E_ROOM for an image whose stream is longer than slot_bytes:
 *                its slot is left untouched, lengths[i] is the size it needs, the other images are not disturbed
 * mmh_png_encode_slot_bytes(H, W) is a slot size no image can exceed (9 bits per filtered byte plus the block headers; it is
 * derived in csrc/png_deflate.h), -1 for sizes the encoder rejects.  Host-side argument errors (N < 0, H or W < 1,
 * H * (1 + 3 W) >= 2^31, slot_bytes < 8, a null pointer or a misaligned scratch with N > 0) return non-zero before any launch.
 * The container (signature, IHDR, chunk CRCs) is the host's: mmhand_amd/png.py.                                              */
enum { MMH_PNGENC_OK = 0, MMH_PNGENC_E_ROOM = 1 };
int64_t mmh_png_encode_slot_bytes(int H, int W);          /* host only */
int64_t mmh_png_encode_scratch_bytes(int N, int H, int W);
int mmh_png_encode_batch(const void* pixels /* uint8 [N][H][W][3] */, int N, int H, int W, int bgr, void* scratch,
                         void* streams /* N slots */, int64_t slot_bytes, int64_t* lengths /* [N] */, int32_t* status /* [N] */,
                         mmh_stream_t s);

/* ---- pose distance and exact nearest-pose search (nearest_neighbor_search/nearest_neighbor_search.py:68-83, poseDistance) ----
 * d(u, v) = arccos(clamp(f(u) . f(v), -1, 1)) / pi, f = the reference's identity(): the 20 consecutive joint differences of a
 * [21][3] pose, flattened to 60 values, divided by their float64 2-norm.  The clamp is a stated divergence: the reference
 * returns NaN where rounding puts the cosine above 1 (identical poses).  The reference searches with a pure-Python k-d tree
 * over other features, which is not exact under this distance; here the search is all pairs on the fp64 MFMA with the
 * selection in the epilogue - no Nq x Nc buffer, no atomics.
 *
 * mmh_pose_features (nearest_neighbor_search.py:68-83, identity()): C float64 [N][21][3] -> F float64 [N][64] (60 values +
 *   4 zeros), valid int32 [N]: 0 for a pose with a non-finite coordinate or a zero norm, whose feature row is zero.
 * mmh_pose_knn (nearest_neighbor_search.py:68-83 under the k-d tree's search_knn): for every query the k (1 .. 16) nearest
 *   candidates, ranked by (larger cosine, then smaller candidate index) - a total order, and every cosine is one fixed chain
 *   of MFMAs, so idx and dist are bit-identical for any cand_split.  Invalid candidates and exclude[q] (int32 [Nq] or NULL;
 *   -1 = none) are never returned; an invalid query, or fewer valid candidates than k, leaves the trailing slots at
 *   idx = -1, dist = NaN.  cand_split: candidates per slice (a multiple of 16), 0 = automatic (at most 32 slices); the
 *   slices' lists are merged by a second kernel in slice order.  ws: mmh_pose_knn_ws_bytes(Nq, Nc, k, cand_split) bytes
 *   (slices * Nq * k * 12, rounded up to 256; 0 = the arguments are refused), 8-byte aligned; F 16-byte aligned.
 * mmh_pose_pair_distance (nearest_neighbor_search.py:68-83): d[i] of the pairs (Fa[i], Fb[i]), NaN if either is invalid.
 * Bad arguments (NULL, N < 1, k outside 1 .. 16, cand_split not a multiple of 16) return non-zero before any launch.           */
int mmh_pose_features(const double* C /* [N][21][3] */, int N, double* F /* [N][64] */, int32_t* valid /* [N] */, mmh_stream_t s);
size_t mmh_pose_knn_ws_bytes(int Nq, int Nc, int k, int cand_split);          /* nearest_neighbor_search.py:68-83; host only */
int mmh_pose_knn(const double* Fq, const int32_t* validq, int Nq, const double* Fc, const int32_t* validc, int Nc,
                 const int32_t* exclude /* [Nq] or NULL */, int k, int cand_split, void* ws, int32_t* idx /* [Nq][k] */,
                 double* dist /* [Nq][k] */, mmh_stream_t s);
int mmh_pose_pair_distance(const double* Fa, const int32_t* valida, const double* Fb, const int32_t* validb, int n,
                           double* d /* [n] */, mmh_stream_t s);

/* ---- depth condition rendered from the 3D joints (--depth_source joints, aug --novel) ----
 * The pose-to-depth stage of the reference, baselines/quantitative_on_benchmarks/utils.py:113-124,142-194 (the 21 joints
 * (u, v, depth / 700 * 255) rasterised bone by bone with a depth test), as an analytic rasteriser: every bone is a capsule
 * of `radius` pixels whose depth runs linearly from joint to joint.  The reference's bone-id colours are not drawn.
 *   xyz0, xyz1 float64 [N][21][3] = (u, v, z): u, v in pixels of the H x W output grid, z in depth / 700 * 255 units
 *   radius     pixels, finite, >= 0;   bg: the z of a pixel no bone covers, finite
 * Per sample and integer pixel (x, y) the 20 bones are walked in the order (0,1) (1,2) (2,3) (3,4) (0,5) (5,6) (6,7) (7,8)
 * (0,9) (9,10) (10,11) (11,12) (0,13) (13,14) (14,15) (15,16) (0,17) (17,18) (18,19) (19,20); bone a -> b:
 *   skipped if any of its six coordinates is not finite
 *   dx = bu-au; dy = bv-av; L2 = dx*dx + dy*dy;  px = x-au; py = y-av
 *   t = L2 > 0 ? (px*dx + py*dy) / L2 : 0;  t = t < 0 ? 0 : t;  t = t > 1 ? 1 : t      (a NaN t stays NaN and covers nothing)
 *   cx = px - t*dx; cy = py - t*dy;  covered iff cx*cx + cy*cy <= radius*radius;  z = az + t*(bz-az)
 * all in float64, every operation rounded on its own (no fused multiply-add), IEEE division.  D = the smallest z of the
 * covering bones (a covering bone replaces D if it is the first, or if z < D), bg if there is none - a bone behind bg still
 * wins over the background.  Stored: ((D / 255.0) - 0.5) / 0.5 in float64, cast to fp32 (the only rounding), in three lanes.
 *   out_lanes 8: out = the decode passes' x_d, fp32 [N][H][W][8], in place: xyz0 -> lanes 0..2, xyz1 -> lanes 3..5.  A NULL
 *                xyz leaves its side's lanes (and 6, 7) bit for bit; with both given all eight lanes are written with two
 *                16-byte stores, 6 and 7 as the zeros the decode passes leave there.  At least one side.
 *   out_lanes 4: out = fp32 [N][H][W][4] of its own from xyz0 (xyz1 NULL): lanes 0..2 the value, lane 3 zero - the layout
 *                of x_h1 / x_h2, so the NCHW [N,3,H,W] view is a stride permutation.
 * out 16-byte aligned.  Bones that cannot reach a workgroup's tile are culled by a bounding box grown by more than the
 * arithmetic's rounding; the result does not depend on it.  One launch, no atomics, no workspace.  Bad arguments return
 * non-zero before any launch.                                                                                          */
int mmh_render_pose_depth(const double* xyz0, const double* xyz1, int N, int H, int W, double radius, double bg,
                          float* out, int out_lanes, mmh_stream_t s);

/* ---- hand-pose estimators for PCK (baselines/quantitative_on_benchmarks/hpe_estimator.py:97-143, networks/net_hpm2d.py,
 *      networks/net_hpm3d.py): the passes around their convolutions.  The convolutions themselves are mmh_conv2d_fprop
 *      (zero padding, ReLU) and the pools mmh_maxpool2x2_fwd.                                                            */

/* replaces data/RHD_dataset.py:121,215-227: cv2.normalize(img, None, alpha=1, norm_type=NORM_MINMAX, dtype=CV_32F).
 * src: B images [3][H][W] of any mmh_image_src dtype and strides (scale / offset are not looked at: a min-max normalisation
 * does not change under an affine map of its input, and the stored values are what is exact).  Per image mn / mx = the
 * smallest / largest stored value over all pixels and the three channels together; out [B][H][W][4] fp32 = (float)
 * (((double)v - mn) / ((double)mx - mn)) in lanes 0..2 in the source's channel order, 0 in lane 3; a constant image gives
 * zeros.  One rounding: bit-identical to that expression in numpy float64.  No atomics; the partials of an image are merged
 * in a fixed order.  ws: mmh_hpe_normalize_ws_bytes(B, H, W) bytes (0 = refused), 8-byte aligned; out 16-byte aligned.   */
size_t mmh_hpe_normalize_ws_bytes(int B, int H, int W);
int mmh_hpe_normalize(const mmh_image_src* src, int B, int H, int W, void* ws, size_t ws_bytes, float* out, mmh_stream_t s);

/* an addition (train_hpe --augment_geom / --augment_color): the reference trains its estimators on the files' pixels as they
 * are (RHD_dataset.py:215-263 has no augmentation); this is the conventional one - rotate / scale / shift / flip and a colour
 * jitter - fused with the min-max normalisation above, which has to FOLLOW the colour operations and be taken over the
 * warped output: it cancels every brightness or contrast change that is one affine map of the three channels together.
 *   img    uint8 [B,Hs,Ws,3] BGR, as the loader reads PNGs
 *   xf     device float64 [B,6] = [a00 a01 a02; a10 a11 a12] per image, or NULL = identity (needs Ho == Hs, Wo == Ws)
 *   cm     device float64 [B,9], row-major on (R,G,B), or NULL = identity
 *   gamma  device float64 [B], > 0, or NULL = 1
 *   out    fp32 [B,Ho,Wo,4]: lanes 0..2 = R,G,B, lane 3 = 0 (one 16-byte store per pixel); 16-byte aligned
 * Per image b and output pixel (x, y), everything in float64:
 *  1. sample: the source coordinate, the clamp (edge replicate, a NaN lands on 0), the taps and the weights are exactly
 *     mmh_decode_inputs_affine's (the text at that entry; no fused multiply-add in the coordinate); per channel
 *     (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11) over the four raw bytes gives R, G, B in [0, 255]
 *  2. colour matrix: v_c = (cm[3c]*R + cm[3c+1]*G) + cm[3c+2]*B, each product and sum rounded on its own, clamped to [0, 255]
 *     (a NaN to 0)
 *  3. gamma: if gamma[b] != 1, v_c = 255 * pow(v_c / 255, gamma[b]); if it is 1 (or NULL) pow is not called
 *  4. normalise: mn / mx = the smallest / largest v_c over all output pixels and the three channels of image b;
 *     out = (float)((v - mn) / (mx - mn)), one rounding; mx == mn gives zeros
 * With xf, cm and gamma NULL or identity the result is bit-identical to mmh_hpe_normalize of the same bytes in "bgr_hwc"
 * order; an integer shift, a flip or a quarter turn has weights 0 and a permutation or power-of-two cm is exact.  The matrices
 * and gamma are the caller's to keep finite (gamma positive): nothing they hold can index outside the image.  Two passes over
 * the source (reduce, then recompute and write), partials merged through ws, no atomics; every byte offset is 64-bit.
 * ws: mmh_hpe_augment_normalize_ws_bytes(B, Ho, Wo) bytes (0 = refused), 8-byte aligned as xf, cm and gamma are.  Non-positive
 * sizes, xf == NULL with differing sizes, a workspace that is too small and a misaligned buffer return non-zero before any
 * launch.                                                                                                                  */
size_t mmh_hpe_augment_normalize_ws_bytes(int B, int Ho, int Wo);
int mmh_hpe_augment_normalize(const void* img, int B, int Hs, int Ws, int Ho, int Wo, const double* xf, const double* cm,
                              const double* gamma, void* ws, size_t ws_bytes, float* out, mmh_stream_t s);

/* replaces networks/net_hpm2d.py:69,118 (nn.Upsample(scale_factor=8, mode='bilinear', align_corners=True)) and
 * hpe_estimator.py:127-135 (torch.max of every joint's map, index -> pixel).
 * heat: fp32 [B][h][w][cs], cs >= 21, joints in lanes 0..20.  up: fp32 [B][8h][8w][24], lanes 21..23 zero (the input of
 * Hpm3d).  For output row oy: sy = ((double)(h - 1) / (double)(8h - 1)) * oy, y0 = (int)sy, y1 = min(y0 + 1, h - 1),
 * wy = sy - y0, columns alike; value = (float)((1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11)),
 * every operation in float64 and rounded on its own (no fused multiply-add), one rounding to fp32.
 * arg [B][21][2] int32 = (x, y) of the largest of the ROUNDED fp32 values, the first one in scan order (y, then x) among
 * equals; maxv [B][21] that value.  The reference computes y = index / H and x = index % W from the flat index, which is
 * the same pixel for its square 256 x 256 maps; here y = index / (8w), x = index % (8w) for any shape.  Band partials
 * merged in scan order, no atomics.  ws: mmh_heatmap_upsample_argmax_ws_bytes(B, h, w) bytes (0 = refused).            */
size_t mmh_heatmap_upsample_argmax_ws_bytes(int B, int h, int w);
int mmh_heatmap_upsample_argmax(const float* heat, int B, int h, int w, int cs, float* up, int32_t* arg, float* maxv, void* ws,
                                size_t ws_bytes, mmh_stream_t s);

/* replaces networks/net_hpm3d.py:60-62,110-114 (nn.Linear of the depth head on a handful of rows).
 * y [M][N] = x [M][K] . wt [K][N] + bias [N], fp32, M <= 64, N % 4 == 0; wt is the transpose of nn.Linear's weight; bias
 * may be NULL.  Definition of the sum, whatever the grid: the contraction is cut into mmh_linear_chunks(K) chunks of 256
 * consecutive k; a chunk's sum is one fma chain over its k in ascending order, starting from bias[n] in chunk 0 and from 0
 * in the others; the chunks' sums are added by the library's slab reduction, whose order depends on their number and on the
 * option "slab_reduce_par" (which of its two kernels runs; the parallel one starts from +0, so a sum of -0.0 comes out +0.0).
 * splits: workgroups along the contraction (<= 0: one per chunk) - it changes the schedule and not one bit of y.
 * ws: mmh_linear_fprop_ws_bytes(M, K, N) bytes (0 = refused); wt, bias, y and ws 16-byte aligned.                       */
int mmh_linear_chunks(int K);
size_t mmh_linear_fprop_ws_bytes(int M, int K, int N);
int mmh_linear_fprop(const float* x, const float* wt, const float* bias, float* y, int M, int K, int N, int splits, void* ws,
                     size_t ws_bytes, mmh_stream_t s);

/* ---- Inception score (baselines/quantitative_on_benchmarks/utils.py:12-112,196-232, inception.py): the passes around
 *      Inception-v3's convolutions (csrc/inception.hip) and the rectangular-padding form of the fp32 forward convolution.
 *      The fully connected layer is mmh_linear_fprop.                                                                       */

/* replaces inception.py:275-282,320-321,351-357 (nn.Conv2d with kernel_size (1,7) / (7,1) / (1,3) / (3,1) and padding
 * (0,3) / (3,0) / (0,1) / (1,0)): mmh_conv2d_fprop for fp32 and zero padding with pad_h rows above and below and pad_w
 * columns left and right.  d->pad is not read and d->pad_mode must be MMH_PAD_ZERO; d->Ho == (H + 2 pad_h - kh) / stride + 1
 * and d->Wo alike with pad_w.  Always the direct implicit-GEMM kernels (the option "conv_levels" holds as for
 * mmh_conv2d_fprop), never the 7x7 stem kernel: with pad_h == pad_w == d->pad the result has the bits of mmh_conv2d_fprop
 * wherever that runs the direct kernels itself (everything but the shapes of the fp32 7x7 stems).                         */
int mmh_conv2d_fprop_rect(const mmh_conv_desc* d, int pad_h, int pad_w, const void* x, const void* w, const void* bias,
                          void* y, int act, mmh_stream_t s);

/* replaces utils.py:22-28 (ToPILImage, Resize(299), CenterCrop(299), ToTensor, Normalize) for a batch.
 * src: B images [3][H][W] of any mmh_image_src dtype and strides (scale / offset are not looked at).  A stored value v that is
 * not uint8 becomes the byte aug writes for it, ((v * 0.5f + 0.5f) * 255.0f) rounded to nearest even and clamped to 0..255, in
 * fp32 with every operation rounded on its own; uint8 values are taken as they are.  [The reference hands ToPILImage the
 * generator's [-1, 1] tensor, whose mul(255).byte() wraps negative values; this is the [0, 1] mapping of mmh_image_metrics.]
 * The bytes are resized as PIL.Image.resize(BILINEAR) resizes them (ImagingResample): a horizontal pass to uint8, then a
 * vertical pass over its result, each clip8(((1 << 21) + sum_t pixel[first + t] * coef[t]) >> 22) with an arithmetic shift.
 * The tables are the host's (mmhand_amd/inception.py: pil_bilinear_tables), device memory:
 *   hbounds int32 [rw][2] = (first source column, taps) of resized column j;  hcoef int32 [rw][hks], 22-bit fixed point
 *   vbounds int32 [rh][2], vcoef int32 [rh][vks]: the same for the rows.  Indices are clamped into the image.
 * Only the window rows crop_y .. crop_y + oh - 1 and columns crop_x .. crop_x + ow - 1 of the rh x rw resized image are
 * produced (the centre crop).  lut fp32 [3][256] (device): channel c's value of byte u after ToTensor and Normalize.
 * out: fp32 [B][oh][ow][4], lanes 0..2 = lut[c][byte], lane 3 zero.  Integer arithmetic and a table: bit-identical to PIL
 * plus the table.  ws: mmh_inception_preprocess_ws_bytes(B, H, W, oh, ow) bytes (0 = refused), 4-byte aligned; out 16-byte. */
size_t mmh_inception_preprocess_ws_bytes(int B, int H, int W, int oh, int ow);
int mmh_inception_preprocess(const mmh_image_src* src, int B, int H, int W, const int32_t* hbounds, const int32_t* hcoef, int hks,
                             int rw, const int32_t* vbounds, const int32_t* vcoef, int vks, int rh, int crop_y, int crop_x, int oh,
                             int ow, const float* lut, void* ws, size_t ws_bytes, float* out, mmh_stream_t s);

/* replaces inception.py:131,137,255,333 (F.max_pool2d(x, kernel_size=3, stride=2): mode MMH_POOL_MAX, no padding, output
 * (H - 3) / 2 + 1 rows, H, W >= 3) and inception.py:225,299,379 (F.avg_pool2d(x, kernel_size=3, stride=1, padding=1): mode
 * MMH_POOL_AVG, output H x W, the window's values inside the image summed in row-major order in fp32 and the sum divided by 9
 * - count_include_pad - with a correctly rounded fp32 division).  x: fp32 NHWC, C lanes (C % 4 == 0) from pointer x with pixel
 * stride x_cs; y likewise with y_cs: a pointer into a wider concat buffer writes only its own C lanes.  x, y 16-byte aligned. */
enum { MMH_POOL_MAX = 0, MMH_POOL_AVG = 1, MMH_POOL_AVG_VALID = 2, MMH_POOL_MAX_S1 = 3 };
int mmh_pool3x3_fwd(const float* x, int B, int H, int W, int C, int x_cs, float* y, int y_cs, int mode, mmh_stream_t s);
/* the two further modes are pytorch-fid's departures from torchvision's graph (mmhand_amd/fid.py, variant "fid"), both stride 1,
 * padding 1, output H x W: MMH_POOL_AVG_VALID is MMH_POOL_AVG's sum divided by the number of window pixels inside the image
 * (F.avg_pool2d(..., count_include_pad=False)), the quotient correctly rounded likewise; MMH_POOL_MAX_S1 is the maximum over
 * those pixels (F.max_pool2d(x, kernel_size=3, stride=1, padding=1)).  Modes 0 and 1 and their bits are what they were. */

/* ---- Frechet and Kernel Inception Distance (mmhand_amd/fid.py; csrc/fid.hip).  The reference has neither metric; the
 *      definitions are pytorch-fid's (mu, np.cov(rowvar=False)) and torch-fidelity's KID (kernel (x.y / d + 1)^3).
 *
 * mmh_feature_moments: X fp32 [N][d] row-major (16-byte aligned, d % 4 == 0, N >= 2) -> mean float64 [d], cov float64 [d][d].
 *   mean[j]: float64 sums of 128-row chunks in row order, the chunks added in order, divided once by N.  cov[i][j] =
 *   sum_n c[n][i] c[n][j] / (N - 1) with c = (double)x - mean formed on load: one chain of ceil(N / 4) v_mfma_f64_16x16x4_f64
 *   over the rows in ascending order from a zero accumulator, the same bits wherever the element's tile lies; only the 64 x 64
 *   tiles on or above the diagonal are multiplied and each element is also stored at its mirror.  fp32 -> fp64 and the
 *   products of converted values are exact: the accumulation is the only rounding.  No atomics, no split over N.
 *   ws: mmh_feature_moments_ws_bytes(N, d) bytes (0 = the arguments are refused), 8-byte aligned.
 * mmh_poly_mmd_sums: A fp32 [Na][d], B fp32 [Nb][d]; idxA int32 [S][Ma], idxB int32 [S][Mb] name rows of A and B (the caller
 *   guarantees 0 <= index < Na, Nb).  With a_p = A[idxA[s][p]], b_q = B[idxB[s][q]] and k(x, y) = (t t) t, t = x.y / d + 1.0
 *   (no contraction): out[s] = { sum_{p != q} k(a_p, a_q), sum_{p != q} k(b_p, b_q), sum_{p, q} k(a_p, b_q) }, p != q by
 *   POSITION in the list.  Every dot product is one chain of d / 4 MFMAs in ascending feature order; the Gram tiles never reach
 *   memory: a 64 x 64 tile's sum (lane, butterfly, wave order) goes to the workspace and a second kernel adds a subset's tiles
 *   in an order fixed by (Ma, Mb); the symmetric blocks multiply the upper tiles only and double them.  The launch shape
 *   follows from (S, Ma, Mb, d) alone, so a subset's three sums do not depend on S or on its slot, bit for bit.
 *   ws: mmh_poly_mmd_sums_ws_bytes(S, Ma, Mb) bytes (0 = refused).
 * Bad arguments (NULL, d % 4 != 0, N < 2, S, Ma, Mb < 1, misalignment) return non-zero before any launch.                   */
size_t mmh_feature_moments_ws_bytes(int N, int d);
int mmh_feature_moments(const float* X, int N, int d, double* mean /* [d] */, double* cov /* [d][d] */, void* ws, mmh_stream_t s);
size_t mmh_poly_mmd_sums_ws_bytes(int S, int Ma, int Mb);
int mmh_poly_mmd_sums(const float* A, const float* B, int d, const int32_t* idxA /* [S][Ma] */, const int32_t* idxB /* [S][Mb] */,
                      int S, int Ma, int Mb, double* out /* [S][3] */, void* ws, mmh_stream_t s);

/* ---- LPIPS, the learned perceptual distance (mmhand_amd/lpips.py; csrc/lpips.hip).  The reference has no such metric; the
 *      definition is the `lpips` package's LPIPS(net="vgg", spatial=False) in eval mode (lpips/lpips.py, lpips/
 *      pretrained_networks.py: vgg16).  The VGG-16 trunk is mmh_conv2d_fprop (zero padding, ReLU) and mmh_maxpool2x2_fwd.
 *
 * mmh_lpips_preprocess replaces lpips.py's ScalingLayer (and, for bytes, the package's im2tensor): src = B images [3][H][W] of
 *   any mmh_image_src dtype and strides (scale / offset are not looked at).  v = the stored value for fp32 / bf16 / fp16 - an
 *   image in [-1, 1] as the generator leaves it -, v = u / 255 * 2 - 1 for MMH_U8.  out [B][H][W][4] fp32: lane c < 3 =
 *   (float)((v_c - shift_c) / scale_c), shift = (-.030, -.088, -.188), scale = (.458, .448, .450), each constant the float32
 *   value of its literal widened to float64; float64 arithmetic without fused multiply-add, one rounding; lane 3 zero.
 *   out 16-byte aligned.
 * mmh_lpips_layer replaces, for one tap, lpips.normalize_tensor of both feature maps, the squared difference, the NetLinLayer
 *   (a 1x1 convolution [1,C,1,1] without bias) and spatial_average (lpips.py:9-10,28-30,88-115).  fa, fb: contiguous fp32
 *   [B][H][W][C]; w: fp32 [C] (any sign; all ones = the package's lpips=False form); out: float64 [B].  In float64, per pixel p:
 *     n_a = sqrt(sum_c a_c^2), ah_c = a_c / (n_a + 1e-10), likewise b;  d(p) = sum_c w_c (ah_c - bh_c)^2;
 *     out[b] = (sum_p d(p)) / (H W).
 *   Both maps are read once, 16 bytes per lane and load, several lanes per pixel; the three sums over c are cross-lane
 *   butterflies, a and b through one sequence of operations: mmh_lpips_layer(a, b) == mmh_lpips_layer(b, a) bit for bit.  A
 *   pixel whose vector is all zero contributes through the 1e-10 alone (0 / 1e-10 = 0) and stays finite.  Workgroup k of an
 *   image (at most 1024 of them) sums its pixels and writes one double to the workspace; a finishing launch adds an image's
 *   partials in a fixed order (thread t: t, t + 256, ...; then a tree) and divides once.  The launch shape follows from
 *   (H W, C) alone and the grid is (workgroups, B): out[b] does not depend on B or on the other images, and is bit-identical
 *   run to run.  No atomics.
 *   C % 4 == 0, 4 <= C <= 512, 1 <= B <= 65535, H, W >= 1, B H W C < 2^31.  fa, fb, w 16-byte, out and ws 8-byte aligned.
 *   ws: mmh_lpips_layer_ws_bytes(B, H, W, C) bytes (0 = the shape is refused) = 8 B (workgroups per image).
 * Bad arguments (NULL, a refused shape, a short workspace, misalignment) return non-zero before any launch.                  */
int mmh_lpips_preprocess(const mmh_image_src* src, int B, int H, int W, float* out, mmh_stream_t s);
size_t mmh_lpips_layer_ws_bytes(int B, int H, int W, int C);
int mmh_lpips_layer(const float* fa, const float* fb, const float* w, int B, int H, int W, int C, double* out /* [B] */, void* ws,
                    size_t ws_bytes, mmh_stream_t s);

/* replaces inception.py:168 (F.adaptive_avg_pool2d(x, (1, 1))): x fp32 [B][H][W] pixels of C lanes with pixel stride x_cs ->
 * y fp32 [B][C] = (float)(sum / (H W)), the sum taken in float64 over the pixels in order.  One thread per value, no atomics. */
int mmh_global_avgpool(const float* x, int B, int H, int W, int C, int x_cs, float* y, mmh_stream_t s);

/* replaces utils.py:208-231 (F.softmax, np.mean(part, 0), scipy.stats.entropy(pyx, py) per row) for one group of n rows.
 * logits: fp32 [n][cs], the first `classes` of each row used.  All in float64 [the reference rounds the softmax to fp32 first]:
 * pyx = exp(l - max l) / sum, the sum a fixed tree over 256 strided partials; py [classes] = the mean of pyx over the rows in
 * row order; kl [n] = sum_c pyx log(pyx / py), terms with pyx == 0 are 0, the same tree.  The host takes exp(mean(kl)).  The
 * launch shapes follow from n and classes alone; no atomics.  ws: mmh_inception_score_ws_bytes(n, classes) bytes (0 = refused). */
size_t mmh_inception_score_ws_bytes(int n, int classes);
int mmh_inception_score(const float* logits, int n, int cs, int classes, double* kl, double* py, void* ws, size_t ws_bytes,
                        mmh_stream_t s);

/* ---- training the 2D hand-pose estimator (mmhand_amd/hpe_train.py; csrc/hpe_train.hip).  The reference has the network
 *      (networks/net_hpm2d.py), the target (data/RHD_dataset.py:245-277) and, under hand_pose_estimators/CVPR2020_hpm3d/models/,
 *      its own training loops (hpm2d_model.py, hpm3d_model.py, hpm_model.py); hpm2d_model.py:143-151 is the loss below - the sum
 *      over the stage outputs of nn.MSELoss() against one Gaussian target - with every weight 1000.  The weights' default of 1
 *      is this port's.                                                                                                       */

/* replaces, for all S stage outputs at once (1 <= S <= 8; Hpm2d has 6): nn.Upsample(scale_factor=8, mode='bilinear',
 * align_corners=True) (net_hpm2d.py:69,118), the target of RHD_dataset.py:245-277, nn.MSELoss() and its backward through the
 * upsample.  No full-resolution tensor is written.
 * heat: HOST array of S device pointers, each fp32 [B][h][w][cs], cs >= 21, joints in lanes 0..20.  uv: device float64
 * [B][21][2] = (x, y) on the 8h x 8w grid.  weight: HOST array of S doubles.  loss: device float64 [S].  dheat: NULL (loss
 * only) or a HOST array of S device pointers, each fp32 [B][h][w][dcs], dcs >= 24: lanes 0..20 receive the gradient, lanes
 * 21..23 zeros, no other lane is touched.  Definition, N = B * 21 * 8h * 8w:
 *   up   = the fp32 value mmh_heatmap_upsample_argmax defines (float64 taps, no fused multiply-add, one rounding);
 *   t    = (float)clip(exp(-D2 / 2.0 / sigma / sigma)), D2 = (ox - x)^2 + (oy - y)^2 in float64 without fused multiply-add,
 *          values above 1 -> 1, values below 0.0099 -> 0;  d = (double)up - (double)t;
 *   loss[s] = sum d^2 / N in float64: per low-res pixel and joint over the outputs whose taps 0 are that pixel in ascending
 *          (oy, ox) order, then a fixed tree over a workgroup's 8 pixels x 24 lanes, then the workgroups in a fixed order;
 *   dheat[s][b,y,x,j] = (float) sum over (oy, ox) ascending of (ay * ax) * ((2 weight[s] / N) * d), float64, where ay / ax
 *          is the bilinear weight with which output row oy / column ox reads source row y / column x (both taps added
 *          where they are the same row / column).
 * Gather form, no atomics: bit-identical run to run.  The target of an output pixel is computed once per visit and shared by
 * the S stages; exp is left out only where -D2 / 2 / sigma^2 < -5 (e^-5 = 0.0067, a third under the cut: the target is 0
 * whatever exp returns).  ws: mmh_heatmap_mse_ws_bytes(S, B, h, w) bytes (0 = refused), 8-byte aligned like uv and loss.    */
size_t mmh_heatmap_mse_ws_bytes(int S, int B, int h, int w);
int mmh_heatmap_mse(const float* const* heat, int S, int B, int h, int w, int cs, const double* uv, double sigma,
                    const double* weight, double* loss, float* const* dheat, int dcs, void* ws, size_t ws_bytes, mmh_stream_t s);

/* The estimator's first convolution for training (networks/net_hpm2d.py:40,75: nn.Conv2d(3, 64, 3, padding=1) + ReLU) with
 * float64 accumulation.  x: fp32 [B][H][W][4] (mmh_hpe_normalize's output, lane 3 zero); w: RSCK fp32 [3][3][4][Cout], Cout % 4
 * == 0, Cout <= 256; y: fp32 [B][H][W] pixels of Cout lanes with pixel stride y_cs.  y = (float)(bias + sum x * w): every
 * product of two fp32 values is exact in float64, the products of the taps inside the image are added to (double)bias in
 * ascending (kh, kw, c) order without fused multiply-add, one rounding, then ReLU if act == MMH_ACT_RELU.  The sign of a
 * pre-activation - the ReLU mask the backward reads - is therefore that of exact arithmetic down to 1e-16 of the terms: of all
 * the layers this one's parameter gradients are summed over the fewest terms (27 inputs), and with the fp32 direct kernel one
 * mask that fp32 rounding flips moved them by 4e-5.  Inference (hpe.Hpm2d) stays on mmh_conv2d_fprop; the two
 * outputs differ by fp32 rounding.  x, w, bias and y 16-byte aligned.                                                        */
int mmh_conv3x3_c4_fprop_f64(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cout, int y_cs,
                             int act, mmh_stream_t s);

/* y[p][c] += x[p][c] for `pixels` pixels and c < lanes (lanes % 4 == 0): x / y point at the first lane of the range inside
 * NHWC buffers with pixel strides x_cs / y_cs (multiples of 4; 16-byte aligned pointers).  The backward of the reference's
 * cat((heat, out_0), 1) (net_hpm2d.py:104-116): a stage's input gradient added onto the heat-map and out_0 gradients.       */
int mmh_lane_add(const float* x, int x_cs, float* y, int y_cs, int64_t pixels, int lanes, mmh_stream_t s);

/* ---- training the 3D hand-pose estimator (mmhand_amd/hpe_train.py: Hpm3dTrainer; csrc/hpe3d_train.hip).  The recipe is the
 *      reference's: hand_pose_estimators/CVPR2020_hpm3d/models/hpm3d_model.py:73,91-113 trains Hpm3d(21, 21) on the ground-truth
 *      heat maps against the labels' depth with nn.SmoothL1Loss() * 10 and Adam.  No atomics in any of the four; every output
 *      element is written once, by one thread, with 16-byte stores where the rows are 16-byte aligned; the results do not
 *      depend on the grid and are bit-identical run to run.                                                                */

/* replaces RHD_dataset.py:129-137,192-200,245-277 (gen_heatmap of the 21 joints at full resolution: the input of Hpm3d) and
 * the upload of that tensor.  uv: device float64 [B][21][2] = (x, y) in pixels of the H x W grid.  out: fp32 [B][H][W] pixels
 * of cs lanes (cs >= 24, cs % 4 == 0): lanes 0..20 = t, the target mmh_heatmap_mse defines (one __device__ function serves
 * both: csrc/hpe_target.h) - (float)clip(exp(-D2 / 2.0 / sigma / sigma)), D2 in float64 without fused multiply-add, values
 * above 1 -> 1, values below 0.0099 -> 0, exp left out only where the exponent is below -5 -; lanes 21..23 zeros; no lane
 * >= 24 is touched.  uv 8-byte, out 16-byte aligned.                                                                       */
int mmh_gauss_heatmaps(const double* uv, int B, int H, int W, double sigma, float* out, int cs, mmh_stream_t s);

/* replaces hpm3d_model.py:73,105 (torch.nn.SmoothL1Loss()(output, depth) * 10) and its backward.  pred: fp32 [M][ps], columns
 * 0..n-1 read; target: device float64 [M][n]; M <= 64, n <= 24 <= dcs.  In float64, no fused multiply-add, d = (double)pred -
 * target:  l = |d| < beta ? 0.5 * d * d / beta : |d| - 0.5 * beta  (torch's rule: at |d| == beta the linear branch);
 *   loss[0] = scale * (sum of l in ascending (m, j) order) / (M n);
 *   dpred[m][j] = (float)((scale / (M n)) * (|d| < beta ? d / beta : sign(d))), columns n..23 zeros, no column >= 24 touched.
 * dpred NULL: the loss only.  One workgroup.  loss, target 8-byte, dpred 16-byte aligned; dcs % 4 == 0.                    */
int mmh_smooth_l1(const float* pred, int ps, const double* target, int M, int n, double beta, double scale, double* loss,
                  float* dpred, int dcs, mmh_stream_t s);

/* replaces the backward of net_hpm3d.py:60-62,112-114 (nn.Linear) with respect to its input: dx [M][K], dx[m][k] = sum_n
 * dy[m][n] * wt[k][n], wt in mmh_linear_fprop's layout [K][N]; one fp32 fma chain per element over n ascending from +0.
 * M <= 64, N % 4 == 0.  dy, wt and dx 16-byte aligned.                                                                     */
int mmh_linear_dgrad(const float* dy, const float* wt, float* dx, int M, int K, int N, mmh_stream_t s);

/* replaces the backward of net_hpm3d.py:60-62,112-114 (nn.Linear) with respect to its parameters: dwt [K][N], dwt[k][n] =
 * sum_m x[m][k] * dy[m][n], one fp32 fma chain over m ascending from +0, every element written; db [N] (may be NULL), db[n] =
 * sum_m dy[m][n], plain fp32 adds over m ascending from +0.  M <= 64, N % 4 == 0.  dy, dwt and db 16-byte aligned.          */
int mmh_linear_wgrad(const float* x, const float* dy, float* dwt, float* db, int M, int K, int N, mmh_stream_t s);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* MMHAND_HIP_H */

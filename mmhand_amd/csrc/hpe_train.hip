// Training the 2D hand-pose estimator (mmhand_amd/hpe_train.py), for gfx950: the loss of all its stage outputs in one pass.
//   * heatmap_mse: nn.Upsample(scale_factor=8, bilinear, align_corners=True) of every stage's heat maps (net_hpm2d.py:69,118),
//     the Gaussian target of RHD_dataset.py:245-277, nn.MSELoss() and its backward through the upsample.  No full-resolution
//     tensor is written.  Gather form: thread (low-res pixel (y, x), lane j) owns the outputs whose bilinear taps read (y, x) -
//     four quadrants, (row tap 0 | 1) x (column tap 0 | 1) - and walks them in ascending (oy, ox) order, so its gradient is one
//     float64 chain and there is no atomic.  The target of an output pixel is computed once per visit and used by all S stages.
//     The squared error of an output pixel is counted by the one thread that is its tap (0, 0); a workgroup folds its threads'
//     sums in a fixed tree and a second kernel folds the workgroups in a fixed order.
//   * lane_add: y[p][y_off + c] += x[p][x_off + c] over a lane range of two NHWC buffers with their own pixel strides (the
//     gradient of the cat buffer's lanes onto a dense buffer).
#include <cmath>
#include "common.h"
#include "hpe_target.h"

namespace {

constexpr int UP = 8;            // nn.Upsample(scale_factor=8)
constexpr int HM_J = 21;         // joints
constexpr int HM_C = 24;         // lanes a pixel's threads cover: 21 joints + 3 zeros
constexpr int HM_PX = 8;         // low-res pixels per workgroup
constexpr int HM_TPB = HM_PX * HM_C;   // 192: three waves
constexpr int HM_SMAX = 8;
constexpr int HM_FIN_TPB = 64;

struct HmArgs {
    const float* heat[HM_SMAX];
    float* dheat[HM_SMAX];
    double coef[HM_SMAX];        // 2 weight[s] / N
};

struct UpTap { int i0, i1; double w; };
// the taps of mmh_heatmap_upsample_argmax (hpe.hip): source coordinate = o * (n_src - 1) / (n_out - 1), the ratio taken first
__device__ __forceinline__ UpTap up_tap(int o, int n_src, int n_out) {
#pragma clang fp contract(off)
    const double scale = n_out > 1 ? (double)(n_src - 1) / (double)(n_out - 1) : 0.0;
    const double s = scale * (double)o;
    UpTap t;
    t.i0 = min((int)s, n_src - 1);
    t.i1 = min(t.i0 + 1, n_src - 1);
    t.w = s - (double)t.i0;
    return t;
}

// the first output index whose tap 0 is >= i (tap 0 never decreases along o): an estimate, then steps on up_tap itself
__device__ __forceinline__ int first_out(int i, int n_src, int n_out) {
    if (i <= 0) return 0;
    if (i >= n_src) return n_out;
    int o = (int)((double)i * (double)(n_out - 1) / (double)(n_src - 1));
    o = max(0, min(o, n_out));
    while (o > 0 && up_tap(o - 1, n_src, n_out).i0 >= i) --o;
    while (o < n_out && up_tap(o, n_src, n_out).i0 < i) ++o;
    return o;
}

// one quadrant of a thread's window: the outputs whose row tap QY and column tap QX are (y, x)
template <int S, int QY, int QX>
__device__ __forceinline__ void hm_quadrant(const HmArgs& a, int64_t img, int h, int w, int cs, int y, int x, int c, double ux,
                                            double uy, double sigma, double far2, double (&g)[S], double (&sq)[S]) {
#pragma clang fp contract(off)
    const int Ho = h * UP, Wo = w * UP;
    const int r0 = y - 1 + QY, c0 = x - 1 + QX;          // tap 0 of this quadrant's outputs
    if (r0 < 0 || c0 < 0) return;
    const int oy_lo = first_out(r0, h, Ho), oy_hi = first_out(r0 + 1, h, Ho);
    const int ox_lo = first_out(c0, w, Wo), ox_hi = first_out(c0 + 1, w, Wo);
    if (oy_lo >= oy_hi || ox_lo >= ox_hi) return;
    const int r1 = min(r0 + 1, h - 1), c1 = min(c0 + 1, w - 1);
    double v00[S], v01[S], v10[S], v11[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const float* hb = a.heat[s] + img * h * w * cs + c;
        v00[s] = (double)hb[((int64_t)r0 * w + c0) * cs];
        v01[s] = (double)hb[((int64_t)r0 * w + c1) * cs];
        v10[s] = (double)hb[((int64_t)r1 * w + c0) * cs];
        v11[s] = (double)hb[((int64_t)r1 * w + c1) * cs];
    }
    for (int oy = oy_lo; oy < oy_hi; ++oy) {
        const UpTap ty = up_tap(oy, h, Ho);
        // the weight with which output row oy reads source row y; both taps where they are the same row
        const double ay = QY == 0 ? ty.w : (ty.i1 == y ? (1.0 - ty.w) + ty.w : 1.0 - ty.w);
        for (int ox = ox_lo; ox < ox_hi; ++ox) {
            const UpTap tx = up_tap(ox, w, Wo);
            const double ax = QX == 0 ? tx.w : (tx.i1 == x ? (1.0 - tx.w) + tx.w : 1.0 - tx.w);
            const double t = (double)mmh::hm_target((double)ox, (double)oy, ux, uy, sigma, far2);
            const double aw = ay * ax;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float up = (float)((1.0 - ty.w) * ((1.0 - tx.w) * v00[s] + tx.w * v01[s]) +
                                         ty.w * ((1.0 - tx.w) * v10[s] + tx.w * v11[s]));
                const double d = (double)up - t;
                g[s] = g[s] + aw * (a.coef[s] * d);
                if (QY == 1 && QX == 1) sq[s] = sq[s] + d * d;
            }
        }
    }
}

// workgroup blockIdx.x of image blockIdx.y: HM_PX consecutive low-res pixels x 24 lanes
template <int S>
__global__ void __launch_bounds__(HM_TPB) heatmap_mse_kernel(HmArgs a, int h, int w, int cs, int dcs,
                                                             const double* __restrict__ uv, double sigma, int write_grad,
                                                             double* __restrict__ part) {
    __shared__ double red[HM_TPB];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int c = tid % HM_C, p = blockIdx.x * HM_PX + tid / HM_C;
    const bool live = p < h * w && c < HM_J;
    double g[S], sq[S];
#pragma unroll
    for (int s = 0; s < S; ++s) g[s] = sq[s] = 0.0;
    if (live) {
        const int y = p / w, x = p % w;
        const double ux = uv[((int64_t)b * HM_J + c) * 2], uy = uv[((int64_t)b * HM_J + c) * 2 + 1];
        const double far2 = mmh::hm_far2(sigma);
        hm_quadrant<S, 0, 0>(a, b, h, w, cs, y, x, c, ux, uy, sigma, far2, g, sq);
        hm_quadrant<S, 0, 1>(a, b, h, w, cs, y, x, c, ux, uy, sigma, far2, g, sq);
        hm_quadrant<S, 1, 0>(a, b, h, w, cs, y, x, c, ux, uy, sigma, far2, g, sq);
        hm_quadrant<S, 1, 1>(a, b, h, w, cs, y, x, c, ux, uy, sigma, far2, g, sq);
    }
    if (write_grad && p < h * w) {
#pragma unroll
        for (int s = 0; s < S; ++s) a.dheat[s][((int64_t)b * h * w + p) * dcs + c] = c < HM_J ? (float)g[s] : 0.f;
    }
    const int64_t nblk = (int64_t)gridDim.x * gridDim.y, blk = (int64_t)b * gridDim.x + blockIdx.x;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        __syncthreads();
        red[tid] = sq[s];
        __syncthreads();
        if (tid < HM_TPB - 128) red[tid] = red[tid] + red[tid + 128];      // 192 -> 128, then halves
        __syncthreads();
        for (int n = 64; n > 0; n >>= 1) {
            if (tid < n) red[tid] = red[tid] + red[tid + n];
            __syncthreads();
        }
        if (tid == 0) part[s * nblk + blk] = red[0];
    }
}

// loss[s] = (the workgroups' sums: thread t takes t, t + 64, ... in ascending order, then a fixed tree) / N
__global__ void __launch_bounds__(HM_FIN_TPB) heatmap_mse_final_kernel(const double* __restrict__ part, int64_t nblk, double n,
                                                                       double* __restrict__ loss) {
    __shared__ double red[HM_FIN_TPB];
    const int s = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < nblk; i += HM_FIN_TPB) acc = acc + part[s * nblk + i];
    red[tid] = acc;
    __syncthreads();
    for (int m = HM_FIN_TPB / 2; m > 0; m >>= 1) {
        if (tid < m) red[tid] = red[tid] + red[tid + m];
        __syncthreads();
    }
    if (tid == 0) loss[s] = red[0] / n;
}

int64_t hm_blocks(int h, int w) { return mmh::cdiv((int64_t)h * w, HM_PX); }

bool hm_shape_ok(int S, int B, int h, int w) {
    return S >= 1 && S <= HM_SMAX && B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (int64_t)h * UP * w * UP < (int64_t(1) << 31);
}

template <int S>
void hm_launch(const HmArgs& a, int B, int h, int w, int cs, int dcs, const double* uv, double sigma, int write_grad,
               double* part, hipStream_t st) {
    hipLaunchKernelGGL(heatmap_mse_kernel<S>, dim3((unsigned)hm_blocks(h, w), B), dim3(HM_TPB), 0, st, a, h, w, cs, dcs, uv, sigma,
                       write_grad, part);
}

// ------------------------------------------------------------------------------------------------- lane-range add
constexpr int LA_TPB = 256;

__global__ void __launch_bounds__(LA_TPB) lane_add_kernel(const float* __restrict__ x, int x_cs, float* __restrict__ y, int y_cs,
                                                          int64_t pixels, int q) {
    const int64_t i = (int64_t)blockIdx.x * LA_TPB + threadIdx.x;
    if (i >= pixels * q) return;
    const int64_t p = i / q;
    const int l = (int)(i - p * q) * 4;
    const float4 a = *reinterpret_cast<const float4*>(x + p * x_cs + l);
    float4* o = reinterpret_cast<float4*>(y + p * y_cs + l);
    const float4 v = *o;
    *o = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
}

// ------------------------------------------------------------------------------------------------- the first convolution
constexpr int C1_PX = 16;        // pixels per workgroup
constexpr int C1_TPB = 256;
constexpr int C1_MAXC = 256;     // output lanes: 36 x 256 weights = 36 KB of LDS

// workgroup = 16 consecutive pixels; thread (pixel, quad q) takes lanes 4 q, 4 q + 64, ... of its pixel.  Every product of two
// fp32 values is exact in float64; the 36 of an output are added to (double)bias in ascending (kh, kw, c) order, taps outside
// the image left out, and the sum is rounded once.
__global__ void __launch_bounds__(C1_TPB) conv3x3_c4_f64_kernel(const float4* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y, int H,
                                                                int W, int Cout, int y_cs, int64_t pixels, int relu) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float ws[];       // [36][Cout]
    const int tid = threadIdx.x;
    for (int i = tid; i < 36 * Cout / 4; i += C1_TPB) reinterpret_cast<float4*>(ws)[i] = reinterpret_cast<const float4*>(w)[i];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * C1_PX + tid / 16;
    if (p >= pixels) return;
    const int px = (int)(p % W), py = (int)((p / W) % H);
    float4 v[9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        in[t] = py + dy >= 0 && py + dy < H && px + dx >= 0 && px + dx < W;
        v[t] = in[t] ? x[p + (int64_t)dy * W + dx] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int c = (tid % 16) * 4; c < Cout; c += 64) {
        const float4 b4 = *reinterpret_cast<const float4*>(bias + c);
        double acc[4] = {(double)b4.x, (double)b4.y, (double)b4.z, (double)b4.w};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (!in[t]) continue;
            const float xs[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const float4 w4 = *reinterpret_cast<const float4*>(ws + (t * 4 + ci) * Cout + c);
                acc[0] = acc[0] + (double)xs[ci] * (double)w4.x;
                acc[1] = acc[1] + (double)xs[ci] * (double)w4.y;
                acc[2] = acc[2] + (double)xs[ci] * (double)w4.z;
                acc[3] = acc[3] + (double)xs[ci] * (double)w4.w;
            }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (float)acc[e];
            if (relu) o[e] = o[e] > 0.f ? o[e] : 0.f;
        }
        *reinterpret_cast<float4*>(y + p * y_cs + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace

int mmh_conv3x3_c4_fprop_f64(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cout, int y_cs,
                             int act, mmh_stream_t s) {
    MMH_REQUIRE(x && w && bias && y, "mmh_conv3x3_c4_fprop_f64: NULL argument");
    MMH_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cout >= 4 && Cout % 4 == 0 && Cout <= C1_MAXC && y_cs >= Cout && y_cs % 4 == 0 &&
                    (int64_t)B * H * W * y_cs < (int64_t(1) << 40) && (int64_t)B * H * W < (int64_t(1) << 31) * C1_PX,
                "mmh_conv3x3_c4_fprop_f64: bad shape B=%d H=%d W=%d Cout=%d y_cs=%d (Cout %% 4 == 0, Cout <= 256)", B, H, W, Cout, y_cs);
    MMH_REQUIRE(act == MMH_ACT_NONE || act == MMH_ACT_RELU, "mmh_conv3x3_c4_fprop_f64: act %d: none | relu", act);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias) |
                  reinterpret_cast<uintptr_t>(y)) & 15) == 0, "mmh_conv3x3_c4_fprop_f64: x, w, bias and y must be 16-byte aligned");
    const int64_t pixels = (int64_t)B * H * W;
    hipLaunchKernelGGL(conv3x3_c4_f64_kernel, dim3((unsigned)mmh::cdiv(pixels, C1_PX)), dim3(C1_TPB), 36 * Cout * sizeof(float),
                       mmh::as_stream(s), reinterpret_cast<const float4*>(x), w, bias, y, H, W, Cout, y_cs, pixels,
                       act == MMH_ACT_RELU ? 1 : 0);
    return mmh::check_launch("conv3x3_c4_f64");
}

size_t mmh_heatmap_mse_ws_bytes(int S, int B, int h, int w) {
    if (!hm_shape_ok(S, B, h, w)) return 0;
    return (size_t)S * B * hm_blocks(h, w) * sizeof(double);
}

int mmh_heatmap_mse(const float* const* heat, int S, int B, int h, int w, int cs, const double* uv, double sigma,
                    const double* weight, double* loss, float* const* dheat, int dcs, void* ws, size_t ws_bytes, mmh_stream_t s) {
    MMH_REQUIRE(heat && uv && weight && loss && ws, "mmh_heatmap_mse: NULL argument");
    MMH_REQUIRE(hm_shape_ok(S, B, h, w), "mmh_heatmap_mse: bad shape S=%d B=%d h=%d w=%d (1 <= S <= 8)", S, B, h, w);
    MMH_REQUIRE(cs >= HM_J && (int64_t)B * h * w * cs < (int64_t(1) << 40), "mmh_heatmap_mse: bad pixel stride cs=%d (cs >= 21)", cs);
    MMH_REQUIRE(!dheat || (dcs >= HM_C && (int64_t)B * h * w * dcs < (int64_t(1) << 40)),
                "mmh_heatmap_mse: bad gradient pixel stride dcs=%d (dcs >= 24)", dcs);
    MMH_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "mmh_heatmap_mse: sigma must be positive and finite");
    const size_t need = mmh_heatmap_mse_ws_bytes(S, B, h, w);
    MMH_REQUIRE(ws_bytes >= need, "mmh_heatmap_mse: workspace %zu bytes < %zu", ws_bytes, need);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(uv) | reinterpret_cast<uintptr_t>(loss)) & 7) == 0,
                "mmh_heatmap_mse: uv, loss and ws must be 8-byte aligned");
    HmArgs a = {};
    const double n = (double)B * HM_J * (double)(h * UP) * (double)(w * UP);
    for (int i = 0; i < S; ++i) {
        MMH_REQUIRE(heat[i] && (!dheat || dheat[i]), "mmh_heatmap_mse: NULL pointer for stage %d", i);
        MMH_REQUIRE(std::isfinite(weight[i]), "mmh_heatmap_mse: weight[%d] is not finite", i);
        MMH_REQUIRE(((reinterpret_cast<uintptr_t>(heat[i]) | (dheat ? reinterpret_cast<uintptr_t>(dheat[i]) : 0)) & 3) == 0,
                    "mmh_heatmap_mse: stage %d is not 4-byte aligned", i);
        a.heat[i] = heat[i];
        a.dheat[i] = dheat ? dheat[i] : nullptr;
        a.coef[i] = 2.0 * weight[i] / n;
    }
    hipStream_t st = mmh::as_stream(s);
    double* part = static_cast<double*>(ws);
    const int wg = dheat ? 1 : 0;
    switch (S) {
        case 1: hm_launch<1>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        case 2: hm_launch<2>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        case 3: hm_launch<3>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        case 4: hm_launch<4>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        case 5: hm_launch<5>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        case 6: hm_launch<6>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        case 7: hm_launch<7>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
        default: hm_launch<8>(a, B, h, w, cs, dcs, uv, sigma, wg, part, st); break;
    }
    if (int rc = mmh::check_launch("heatmap_mse")) return rc;
    hipLaunchKernelGGL(heatmap_mse_final_kernel, dim3(S), dim3(HM_FIN_TPB), 0, st, part, (int64_t)B * hm_blocks(h, w), n, loss);
    return mmh::check_launch("heatmap_mse_final");
}

int mmh_lane_add(const float* x, int x_cs, float* y, int y_cs, int64_t pixels, int lanes, mmh_stream_t s) {
    MMH_REQUIRE(x && y, "mmh_lane_add: NULL argument");
    MMH_REQUIRE(pixels >= 1 && lanes >= 4 && lanes % 4 == 0 && x_cs >= lanes && y_cs >= lanes && x_cs % 4 == 0 && y_cs % 4 == 0 &&
                    pixels * (int64_t)lanes / 4 < (int64_t(1) << 31) * LA_TPB,
                "mmh_lane_add: bad shape pixels=%lld lanes=%d x_cs=%d y_cs=%d (multiples of 4)", (long long)pixels, lanes, x_cs, y_cs);
    MMH_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0,
                "mmh_lane_add: x and y must be 16-byte aligned");
    const int q = lanes / 4;
    hipLaunchKernelGGL(lane_add_kernel, dim3((unsigned)mmh::cdiv(pixels * q, LA_TPB)), dim3(LA_TPB), 0, mmh::as_stream(s), x, x_cs, y,
                       y_cs, pixels, q);
    return mmh::check_launch("lane_add");
}

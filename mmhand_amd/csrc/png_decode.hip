// mmh_png_decode_batch: N PNG images (their concatenated IDAT payloads) -> uint8 [N,H,W,3], one 64-lane workgroup per image.
//
// Phase 1 + 2, inflate and Adler-32: png_inflate.h with 64 lanes.  The wave stages the stream into LDS 4 KiB at a time (all
// lanes load aligned dwords), builds the block's Huffman tables in LDS, decodes symbols wave-uniformly (every lane walks the
// same bits: LDS broadcast reads, no divergence, no cross-lane traffic), copies matches and stored bytes with all lanes into a
// 32 KiB LDS window and flushes the window to the image's scratch slot 8 KiB at a time (16-byte stores when the slot is
// aligned), summing the Adler-32 terms of the piece on the way out.
// Phase 3, unfilter: rows in bands of 64, lane = row, as a skewed wavefront - at step t lane l reconstructs pixel t - l of its
// row; "up" is what lane l - 1 produced one step earlier and "up-left" what it produced two steps earlier, both by one
// cross-lane move per step, so every filter type (the recurrences Avg and Paeth as well as None / Sub / Up) runs in the same
// W + 63 steps per band and mixed per-row filters cost nothing extra.  Lane 0's row above is the last row of the previous
// band, read back from `out`, 64 pixels at a time.
#include "common.h"
#include "png_inflate.h"

namespace {

using namespace mmh_png;

struct WaveLanes {
    static constexpr uint32_t N = 64;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t sum(uint32_t v) const {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
};

__device__ __forceinline__ uint32_t load_px(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }

__device__ __forceinline__ void unfilter_image(const uint8_t* scr, uint8_t* out, int H, int W, int bgr) {
    const uint32_t stride = 1 + 3 * (uint32_t)W;
    const int lane = threadIdx.x;
    for (int r0 = 0; r0 < H; r0 += 64) {
        __syncthreads();                                   // the previous band's rows are in `out`
        const int r = r0 + lane;
        const bool active = r < H;
        const uint8_t* row = scr + (size_t)(active ? r : 0) * stride;
        uint8_t* orow = out + (size_t)(active ? r : 0) * W * 3;
        const uint8_t* above = out + (size_t)(r0 ? r0 - 1 : 0) * W * 3;
        const uint32_t ft = active ? row[0] : 0;
        uint32_t left = 0, upleft = 0, upchunk = 0, raw4[4] = {0, 0, 0, 0};
        const int steps = W + 63;
        for (int t = 0; t < steps; ++t) {
            if ((t & 63) == 0) {                           // pixels t .. t + 63 of the row above the band, one per lane, as R | G << 8 | B << 16
                const int xa = t + lane;
                upchunk = 0;
                if (r0 > 0 && xa < W) {
                    const uint32_t p = load_px(above + (size_t)xa * 3);
                    upchunk = bgr ? ((p & 0xff) << 16 | (p & 0xff00) | (p >> 16)) : p;
                }
            }
            const int x = t - lane;
            if ((x & 3) == 0 || t == 0) {                  // this lane's next four filtered pixels
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int xq = (x & ~3) + q;
                    raw4[q] = (active && xq >= 0 && xq < W) ? load_px(row + 1 + (size_t)xq * 3) : 0;
                }
            }
            uint32_t up = __shfl_up(left, 1, 64);
            const uint32_t up0 = __shfl(upchunk, t & 63, 64);
            if (lane == 0) up = up0;
            const bool valid = active && x >= 0 && x < W;
            if (valid) {
                const uint32_t f = raw4[x & 3];
                uint32_t px = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    px |= unfilter_byte(ft, (f >> (8 * c)) & 255, (left >> (8 * c)) & 255, (up >> (8 * c)) & 255,
                                        (upleft >> (8 * c)) & 255) << (8 * c);
                uint8_t* o = orow + (size_t)x * 3;
                o[bgr ? 2 : 0] = (uint8_t)px;
                o[1] = (uint8_t)(px >> 8);
                o[bgr ? 0 : 2] = (uint8_t)(px >> 16);
                left = px;
            }
            upleft = up;
        }
    }
}

__global__ void __launch_bounds__(64) png_decode_kernel(const uint8_t* __restrict__ streams, int64_t streams_bytes,
                                                        const int64_t* __restrict__ offsets, int H, int W,
                                                        uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
                                                        int32_t* __restrict__ status, int bgr) {
    __shared__ Shared sh;
    const int img = blockIdx.x;
    const int64_t beg = offsets[img], end = offsets[img + 1];
    const uint32_t stride = 1 + 3 * (uint32_t)W, total = (uint32_t)H * stride;
    uint8_t* scr = scratch + (size_t)img * total;
    int rc;
    if (beg < 0 || end < beg || end > streams_bytes) {
        rc = MMH_PNG_E_RANGE;
    } else {
        Inflater<WaveLanes> inf(WaveLanes(), sh, streams, beg, end, scr, total);
        rc = inf.run();
    }
    if (rc == 0) {
        __syncthreads();                                   // the scratch slot is complete (written by this wave)
        int bad = 0;
        for (int r = threadIdx.x; r < H; r += 64) bad |= scr[(size_t)r * stride] > 4;
        if (__syncthreads_or(bad)) rc = MMH_PNG_E_FILTER;
    }
    if (rc == 0) unfilter_image(scr, out + (size_t)img * H * W * 3, H, W, bgr);
    if (threadIdx.x == 0) status[img] = rc;
}

}  // namespace

extern "C" int mmh_png_decode_batch(const void* streams, int64_t streams_bytes, const int64_t* offsets, int N, int H, int W,
                                    void* scratch, void* out, int32_t* status, int bgr, mmh_stream_t s) {
    MMH_REQUIRE(N >= 0 && H >= 1 && W >= 1, "mmh_png_decode_batch: N >= 0, H >= 1, W >= 1 (got %d, %d, %d)", N, H, W);
    MMH_REQUIRE((int64_t)H * (1 + 3 * (int64_t)W) < (1ll << 31), "mmh_png_decode_batch: H * (1 + 3 W) must stay below 2^31");
    if (N == 0) return 0;
    MMH_REQUIRE(streams && offsets && scratch && out && status && streams_bytes >= 0,
                "mmh_png_decode_batch: null buffer or negative streams_bytes");
    hipLaunchKernelGGL(png_decode_kernel, dim3(N), dim3(64), 0, mmh::as_stream(s), (const uint8_t*)streams, streams_bytes,
                       offsets, H, W, (uint8_t*)scratch, (uint8_t*)out, status, bgr);
    return mmh::check_launch("mmh_png_decode_batch");
}

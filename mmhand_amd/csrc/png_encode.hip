// mmh_png_encode_batch: uint8 [N,H,W,3] -> N zlib streams (the IDAT payload of an 8-bit RGB PNG), png_deflate.h with 256 lanes.
//
// Two launches over (image, segment of 16 rows), so 64 images of 256 x 256 are 1024 workgroups, not 64 waves:
//   png_encode_a_kernel  filters the segment's rows (lanes stride over the row's pixels, the five filters' sums meet in LDS
//                        integer atomics), histograms the filtered bytes in LDS, builds the segment's Huffman code (a rank
//                        sort by all lanes, the two-queue merge by one) and writes the filtered rows and the segment's META
//                        words (bit count, header bits, code table, Adler-32 partial, last 7 bits) to scratch;
//   png_encode_c_kernel  sums the image's bit counts (its own offset and the total), scans the code lengths of 2048 symbols at
//                        a time across the workgroup, ORs the codes into an LDS staging buffer and stores the complete bytes;
//                        the image's last workgroup adds the pad, the Adler-32 trailer, lengths[i] and status[i].
// The kernel boundary is the only hand-off between workgroups; inside a launch a workgroup reads only what it wrote itself.
// Every output byte has one owner (png_deflate.h), so no global atomics and nothing to zero between batches.
#include "common.h"
#include "png_deflate.h"

namespace {

using namespace mmh_png;

struct BlockLanes {
    static constexpr uint32_t N = 256;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void add32(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
    __device__ __forceinline__ void add64(uint64_t* p, uint64_t v) const {
        atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
    }
    __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
};

__global__ void __launch_bounds__(256) png_encode_a_kernel(const uint8_t* __restrict__ pixels, int H, int W, int bgr, int64_t nseg,
                                                           uint32_t* __restrict__ metas, uint8_t* __restrict__ filt) {
    __shared__ EncShared<256> sh;
    const int64_t img = blockIdx.x / nseg, seg = blockIdx.x % nseg;
    const int64_t raw = (int64_t)H * (1 + 3 * (int64_t)W);
    enc_pass_a(BlockLanes(), sh, pixels + img * H * W * 3, H, W, bgr, seg, nseg, filt + img * raw,
               metas + (img * nseg + seg) * ENC_META_WORDS);
}

__global__ void __launch_bounds__(256) png_encode_c_kernel(int H, int W, int64_t nseg, const uint32_t* __restrict__ metas,
                                                           const uint8_t* __restrict__ filt, uint8_t* __restrict__ streams,
                                                           int64_t slot_bytes, int64_t* __restrict__ lengths,
                                                           int32_t* __restrict__ status) {
    __shared__ EncShared<256> sh;
    const int64_t img = blockIdx.x / nseg, seg = blockIdx.x % nseg;
    const int64_t raw = (int64_t)H * (1 + 3 * (int64_t)W);
    enc_pass_c(BlockLanes(), sh, H, W, seg, nseg, filt + img * raw, metas + img * nseg * ENC_META_WORDS, streams + img * slot_bytes,
               slot_bytes, lengths + img, status + img);
}

}  // namespace

extern "C" int64_t mmh_png_encode_slot_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * (1 + 3 * (int64_t)W) >= (1ll << 31)) return -1;
    return enc_slot_bytes(H, W);
}

extern "C" int64_t mmh_png_encode_scratch_bytes(int N, int H, int W) {
    if (N < 0 || H < 1 || W < 1 || (int64_t)H * (1 + 3 * (int64_t)W) >= (1ll << 31)) return -1;
    return enc_scratch_bytes(N, H, W);
}

extern "C" int mmh_png_encode_batch(const void* pixels, int N, int H, int W, int bgr, void* scratch, void* streams,
                                    int64_t slot_bytes, int64_t* lengths, int32_t* status, mmh_stream_t s) {
    MMH_REQUIRE(N >= 0 && H >= 1 && W >= 1, "mmh_png_encode_batch: N >= 0, H >= 1, W >= 1 (got %d, %d, %d)", N, H, W);
    MMH_REQUIRE((int64_t)H * (1 + 3 * (int64_t)W) < (1ll << 31), "mmh_png_encode_batch: H * (1 + 3 W) must stay below 2^31");
    MMH_REQUIRE(slot_bytes >= 8, "mmh_png_encode_batch: slot_bytes must be at least 8");
    if (N == 0) return 0;
    MMH_REQUIRE(pixels && scratch && streams && lengths && status, "mmh_png_encode_batch: null buffer");
    MMH_REQUIRE(((uintptr_t)scratch & 15) == 0, "mmh_png_encode_batch: scratch must be 16-byte aligned");
    const int64_t nseg = enc_nseg(H), blocks = nseg * N;
    MMH_REQUIRE(blocks < (1ll << 31), "mmh_png_encode_batch: N * ceil(H / 16) must stay below 2^31");
    uint32_t* metas = (uint32_t*)scratch;
    uint8_t* filt = (uint8_t*)scratch + enc_meta_bytes(N, H);
    hipLaunchKernelGGL(png_encode_a_kernel, dim3((unsigned)blocks), dim3(256), 0, mmh::as_stream(s), (const uint8_t*)pixels, H, W,
                       bgr, nseg, metas, filt);
    hipLaunchKernelGGL(png_encode_c_kernel, dim3((unsigned)blocks), dim3(256), 0, mmh::as_stream(s), H, W, nseg,
                       (const uint32_t*)metas, (const uint8_t*)filt, (uint8_t*)streams, slot_bytes, lengths, status);
    return mmh::check_launch("mmh_png_encode_batch");
}

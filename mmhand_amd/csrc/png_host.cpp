// libmmhand_png_host.so: the decoder core of png_inflate.h compiled for the host with one lane, plus a scalar unfilter, and
// the encoder core of png_deflate.h with one lane.  A TEST ARTEFACT - tests/test_png_cpu.py and tests/test_png_encode_cpu.py
// check the bit-level code (every status, every bounds test) without a GPU through it, and the GPU tests compare the device's
// status codes and streams with it entry for entry.  mmhand_amd/lib.py never loads it: the product path is
// mmh_png_decode_batch / mmh_png_encode_batch of libmmhand_hip.so and has no fallback to this.
#include <cstdlib>
#include <cstring>
#include <new>

#include "png_deflate.h"
#include "png_inflate.h"

using namespace mmh_png;

static thread_local uint64_t g_last_steps = 0;

static int decode_one(Shared& sh, const uint8_t* streams, int64_t beg, int64_t end, int H, int W, uint8_t* scr, uint8_t* out,
                      int bgr) {
    const uint32_t stride = 1 + 3 * (uint32_t)W, total = (uint32_t)H * stride;
    Inflater<HostLanes> inf(HostLanes(), sh, streams, beg, end, scr, total);
    const int rc = inf.run();
    if (inf.steps > g_last_steps) g_last_steps = inf.steps;
    if (rc) return rc;
    for (int r = 0; r < H; ++r)
        if (scr[(size_t)r * stride] > 4) return MMH_PNG_E_FILTER;
    for (int r = 0; r < H; ++r) {
        const uint8_t* row = scr + (size_t)r * stride;
        const uint32_t ft = row[0];
        uint8_t* cur = out + (size_t)r * W * 3;
        const uint8_t* up = r ? cur - (size_t)W * 3 : nullptr;
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < 3; ++c) {
                const int o = bgr ? 2 - c : c;
                const uint32_t a = x ? cur[(x - 1) * 3 + o] : 0, b = up ? up[x * 3 + o] : 0, cc = (up && x) ? up[(x - 1) * 3 + o] : 0;
                cur[x * 3 + o] = (uint8_t)unfilter_byte(ft, row[1 + 3 * x + c], a, b, cc);
            }
    }
    return 0;
}

extern "C" {
#pragma GCC visibility push(default)
// the arguments of mmh_png_decode_batch, all pointers host memory, the stream ignored
int mmh_png_decode_batch_host(const void* streams, int64_t streams_bytes, const int64_t* offsets, int N, int H, int W,
                              void* scratch, void* out, int32_t* status, int bgr, void* stream) {
    (void)stream;
    if (N < 0 || H < 1 || W < 1 || (int64_t)H * (1 + 3 * (int64_t)W) >= (1ll << 31)) return 1;
    if (N == 0) return 0;
    if (!streams || !offsets || !scratch || !out || !status || streams_bytes < 0) return 1;
    Shared* sh = new (std::nothrow) Shared;
    if (!sh) return 1;
    g_last_steps = 0;
    const size_t raw = (size_t)H * (1 + 3 * (size_t)W);
    for (int i = 0; i < N; ++i) {
        const int64_t b = offsets[i], e = offsets[i + 1];
        if (b < 0 || e < b || e > streams_bytes) { status[i] = MMH_PNG_E_RANGE; continue; }
        status[i] = decode_one(*sh, (const uint8_t*)streams, b, e, H, W, (uint8_t*)scratch + raw * i,
                               (uint8_t*)out + (size_t)H * W * 3 * i, bgr);
    }
    delete sh;
    return 0;
}
// the bound on the decoder's loop iterations for one image, and the largest count an image of this thread's last call took
uint64_t mmh_png_host_step_bound(uint64_t in_bytes, uint64_t raw_bytes) { return max_steps(in_bytes, raw_bytes); }
uint64_t mmh_png_host_last_steps(void) { return g_last_steps; }
// the arguments of mmh_png_encode_batch, all pointers host memory, the stream ignored
int mmh_png_encode_batch_host(const void* pixels, int N, int H, int W, int bgr, void* scratch, void* streams, int64_t slot_bytes,
                              int64_t* lengths, int32_t* status, void* stream) {
    (void)stream;
    if (N < 0 || H < 1 || W < 1 || (int64_t)H * (1 + 3 * (int64_t)W) >= (1ll << 31) || slot_bytes < 8) return 1;
    if (N == 0) return 0;
    if (!pixels || !scratch || !streams || !lengths || !status || ((uintptr_t)scratch & 15)) return 1;
    EncShared<1>* sh = new (std::nothrow) EncShared<1>;
    if (!sh) return 1;
    const int64_t nseg = enc_nseg(H), raw = (int64_t)H * (1 + 3 * (int64_t)W);
    uint32_t* metas = (uint32_t*)scratch;
    uint8_t* filt = (uint8_t*)scratch + enc_meta_bytes(N, H);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t g = 0; g < nseg; ++g)
            enc_pass_a(HostEncLanes(), *sh, (const uint8_t*)pixels + i * H * W * 3, H, W, bgr, g, nseg, filt + i * raw,
                       metas + (i * nseg + g) * ENC_META_WORDS);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t g = 0; g < nseg; ++g)
            enc_pass_c(HostEncLanes(), *sh, H, W, g, nseg, filt + i * raw, metas + i * nseg * ENC_META_WORDS,
                       (uint8_t*)streams + i * slot_bytes, slot_bytes, lengths + i, status + i);
    delete sh;
    return 0;
}
int64_t mmh_png_encode_host_slot_bytes(int H, int W) { return enc_slot_bytes(H, W); }
int64_t mmh_png_encode_host_scratch_bytes(int N, int H, int W) { return enc_scratch_bytes(N, H, W); }
int mmh_png_encode_host_seg_rows(void) { return ENC_SEG_ROWS; }
#pragma GCC visibility pop
}

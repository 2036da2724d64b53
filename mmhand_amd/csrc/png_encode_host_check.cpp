// make png_encode_host_check: the encoder core of png_deflate.h, one lane, under ASan + UBSan in a program of its own (no
// Python: sanitized code is not loaded into an interpreter).  Every buffer is a heap allocation of exactly the size the
// interface promises - scratch, N slots, lengths, status - so one byte out of bounds is a report.  Cases: uniform noise (the
// longest streams), a one-row image whose histogram forces the 15-bit limit, ragged sizes (1 x 1, 5 x 7, 129 x 65, 33 x 17),
// flat rows; each encoded with the slot bound, then with slots of exactly the longest stream (tight), then one byte short of
// it (that image must report MMH_PNGENC_E_ROOM and write nothing).  Every stream is inflated by the project's own decoder
// core (png_inflate.h) and unfiltered back to the input.  Exit status 0 and "ok" = clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_deflate.h"

using namespace mmh_png;

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

struct Run {
    std::vector<int64_t> lengths;
    std::vector<int32_t> status;
    uint8_t* streams;
    int64_t slot;
};

static Run encode(const uint8_t* px, int N, int H, int W, int bgr, int64_t slot, EncShared<1>& sh) {
    const int64_t nseg = enc_nseg(H), raw = (int64_t)H * (1 + 3 * (int64_t)W);
    // aligned_alloc: the interface asks for a 16-byte aligned scratch
    const size_t sbytes = (size_t)enc_scratch_bytes(N, H, W);
    uint8_t* scratch = (uint8_t*)std::aligned_alloc(16, (sbytes + 15) & ~(size_t)15);
    Run r;
    r.slot = slot;
    r.streams = (uint8_t*)std::malloc((size_t)(N * slot));
    std::memset(r.streams, 0xC3, (size_t)(N * slot));
    r.lengths.assign(N, -1);
    r.status.assign(N, -1);
    uint32_t* metas = (uint32_t*)scratch;
    uint8_t* filt = scratch + enc_meta_bytes(N, H);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t g = 0; g < nseg; ++g)
            enc_pass_a(HostEncLanes(), sh, px + i * H * W * 3, H, W, bgr, g, nseg, filt + i * raw, metas + (i * nseg + g) * ENC_META_WORDS);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t g = 0; g < nseg; ++g)
            enc_pass_c(HostEncLanes(), sh, H, W, g, nseg, filt + i * raw, metas + i * nseg * ENC_META_WORDS, r.streams + i * slot, slot,
                       &r.lengths[i], &r.status[i]);
    std::free(scratch);
    return r;
}

// inflate + unfilter image i of a run and compare with the pixels
static void verify(const Run& r, int i, const uint8_t* px, int H, int W, int bgr, Shared& dsh, const char* what) {
    const uint32_t stride = 1 + 3 * (uint32_t)W, total = (uint32_t)H * stride;
    std::vector<uint8_t> scr(total);
    Inflater<HostLanes> inf(HostLanes(), dsh, r.streams, i * r.slot, i * r.slot + r.lengths[i], scr.data(), total);
    const int rc = inf.run();
    CHECK(rc == 0, "%s: image %d does not inflate (status %d)", what, i, rc);
    if (rc) return;
    std::vector<uint8_t> out((size_t)H * W * 3);
    for (int y = 0; y < H; ++y) {
        const uint8_t* row = scr.data() + (size_t)y * stride;
        CHECK(row[0] <= 4, "%s: filter byte %d", what, row[0]);
        if (row[0] > 4) return;
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < 3; ++c) {
                const size_t o = ((size_t)y * W + x) * 3 + c;
                const uint32_t a = x ? out[o - 3] : 0, b = y ? out[o - (size_t)W * 3] : 0, cc = (x && y) ? out[o - (size_t)W * 3 - 3] : 0;
                out[o] = (uint8_t)unfilter_byte(row[0], row[1 + 3 * x + c], a, b, cc);
            }
    }
    const uint8_t* src = px + (size_t)i * H * W * 3;
    for (size_t k = 0; k < out.size(); ++k) {
        const size_t s = bgr ? k - k % 3 + (2 - k % 3) : k;
        if (out[k] != src[s]) { CHECK(false, "%s: image %d differs at byte %zu", what, i, k); return; }
    }
}

static void run_case(const char* what, const std::vector<uint8_t>& px, int N, int H, int W, EncShared<1>& sh, Shared& dsh) {
    for (int bgr = 0; bgr < 2; ++bgr) {
        const int64_t bound = enc_slot_bytes(H, W);
        Run full = encode(px.data(), N, H, W, bgr, bound, sh);
        int64_t longest = 0;
        for (int i = 0; i < N; ++i) {
            CHECK(full.status[i] == MMH_PNGENC_OK && full.lengths[i] >= 8 && full.lengths[i] <= bound, "%s: status %d length %lld bound %lld",
                  what, full.status[i], (long long)full.lengths[i], (long long)bound);
            if (full.status[i] == MMH_PNGENC_OK) verify(full, i, px.data(), H, W, bgr, dsh, what);
            if (full.lengths[i] > longest) longest = full.lengths[i];
        }
        Run tight = encode(px.data(), N, H, W, bgr, longest, sh);           // the longest stream fills its slot to the last byte
        for (int i = 0; i < N; ++i) {
            CHECK(tight.status[i] == MMH_PNGENC_OK && tight.lengths[i] == full.lengths[i], "%s: tight slot, image %d", what, i);
            CHECK(std::memcmp(tight.streams + i * longest, full.streams + i * bound, (size_t)full.lengths[i]) == 0, "%s: tight bytes", what);
        }
        if (longest > 8) {
            Run shortr = encode(px.data(), N, H, W, bgr, longest - 1, sh);     // one byte short: no room for the longest
            for (int i = 0; i < N; ++i) {
                const bool fits = full.lengths[i] <= longest - 1;
                CHECK(shortr.status[i] == (fits ? MMH_PNGENC_OK : MMH_PNGENC_E_ROOM), "%s: short slot, image %d status %d", what, i, shortr.status[i]);
                if (!fits) {
                    CHECK(shortr.lengths[i] == full.lengths[i], "%s: the needed size", what);
                    for (int64_t k = 0; k < longest - 1; ++k)
                        if (shortr.streams[i * (longest - 1) + k] != 0xC3) { CHECK(false, "%s: a slot without room was written", what); break; }
                }
            }
            std::free(shortr.streams);
        }
        std::free(tight.streams);
        std::free(full.streams);
    }
    std::printf("%-28s N=%d %dx%d\n", what, N, W, H);
}

int main() {
    EncShared<1>* sh = new EncShared<1>;
    Shared* dsh = new Shared;
    const int sizes[][2] = {{1, 1}, {5, 7}, {16, 16}, {33, 17}, {129, 65}, {256, 256}};
    for (auto& wh : sizes) {
        const int W = wh[0], H = wh[1], N = 3;
        std::vector<uint8_t> px((size_t)N * H * W * 3);
        for (auto& v : px) v = (uint8_t)rnd();
        run_case("uniform noise", px, N, H, W, *sh, *dsh);
        for (size_t k = 0; k < px.size(); ++k) px[k] = k < px.size() / 3 ? 200 : (uint8_t)((k / 7) + (rnd() & 3));
        run_case("flat / ramp / noise mix", px, N, H, W, *sh, *dsh);
    }
    {   // one row of 30000 pixels whose Sub residues follow 3 x Fibonacci counts: the code-length limit acts
        const int W = 30000;
        std::vector<uint8_t> res;
        uint32_t f0 = 1, f1 = 1;
        for (uint8_t sym = 1; res.size() < (size_t)3 * W; ++sym) {
            for (uint32_t k = 0; k < 3 * f0 && res.size() < (size_t)3 * W; ++k) res.push_back(sym);
            const uint32_t t = f0 + f1; f0 = f1; f1 = t;
        }
        for (size_t k = res.size() - 1; k > 0; --k) { const size_t j = rnd() % (k + 1); const uint8_t t = res[k]; res[k] = res[j]; res[j] = t; }
        std::vector<uint8_t> px((size_t)3 * W);
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < 3; ++c) px[3 * x + c] = (uint8_t)((x ? px[3 * (x - 1) + c] : 0) + res[3 * x + c]);
        run_case("Fibonacci histogram", px, 1, 1, W, *sh, *dsh);
    }
    delete sh;
    delete dsh;
    std::printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}

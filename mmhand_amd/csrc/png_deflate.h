// The bit-level core of the PNG encoder (png_encode.hip on the device, png_host.cpp on the host): PNG row filters and a
// Huffman-only DEFLATE (RFC 1950 / 1951) of the filtered rows.  ONE implementation for both builds, integer arithmetic only:
// the code is written for `L::N` lanes that run it in lockstep between `sync()`s (a 256-thread workgroup on the device, one
// lane on the host), and everything lanes combine - filter sums, histograms, Adler-32 terms, output words - is an integer sum
// or OR, so the bytes do not depend on the lane count.
//
// An image of H rows is cut into segments of ENC_SEG_ROWS rows (the last one ragged).  Pass A, per (image, segment): choose
// each row's filter (types 0 - 4, smallest sum of |signed byte| over the row's 3 W bytes, ties to the lower type), write the
// filtered rows to scratch, histogram them, build a complete length-limited Huffman code (15 bits; the code-length code 7
// bits), the block header's bits, the block's bit count, its Adler-32 partial and its last 7 bits - all into the segment's
// META words.  Pass C, per (image, segment): the bit offset of the block is 16 + the sum of the earlier blocks' bit counts, so
// every block is emitted at its own offset with no serial dependence.  The output has one owner per BYTE: a block stores the
// bytes [offset / 8, end / 8); the bits of the byte it shares with the previous block are that block's last bits, which it
// reads from the previous META (every block but an image's last has >= 64 symbols, so 7 bits reach back one block only).  The
// last block adds the pad, the Adler-32 trailer, lengths[i] and status[i]; the first one the zlib header.
//
// Bounds, by construction: scratch is written only inside the segment's own rows and META; the slot only at
// [0, need) after need <= slot_bytes was tested (and every store is clamped to slot_bytes again); an image that does not fit
// writes nothing but its status and the size it needs.
#pragma once
#include <stdint.h>

#include "png_inflate.h"

namespace mmh_png {

constexpr int ENC_SEG_ROWS = 16;
constexpr uint32_t ENC_TILE = 2048;                          // symbols emitted per staging round
constexpr uint32_t ENC_OBUF_WORDS = 1024;                    // >= (7 + ENC_TILE * 15) / 32 + 2 and >= the header's words
constexpr uint32_t ENC_HDR_WORDS = 64;
// BFINAL + BTYPE + HLIT + HDIST + HCLEN, 19 code-length code lengths, 258 lengths of at most 7 bits each (a repeat token
// stands for >= 3 lengths and takes <= 7 + 7 bits): no header is longer
constexpr uint32_t ENC_HDR_MAX_BITS = 17 + 19 * 3 + 258 * 7;
enum { EM_BITS_LO = 0, EM_BITS_HI = 1, EM_HDR_BITS = 2, EM_ADLER_A = 3, EM_ADLER_B = 4, EM_TAIL = 5, EM_NBYTES = 6, EM_HDR = 8,
       EM_CODE = EM_HDR + ENC_HDR_WORDS, ENC_META_WORDS = 336 };   // EM_CODE + 257 rounded up to a multiple of 4 words

MMH_HD int64_t enc_nseg(int H) { return ((int64_t)H + ENC_SEG_ROWS - 1) / ENC_SEG_ROWS; }
// A slot size no image of H x W can exceed.  Per block the encoder takes the cheaper of its length-limited code and the flat
// code (literals 0 .. 254 in 8 bits, 255 and end-of-block in 9: Kraft sum 255 / 256 + 2 / 512 = 1), so a block of n bytes
// costs at most ENC_HDR_MAX_BITS + 9 (n + 1) bits whatever the limiter did; the blocks' n sum to H (1 + 3 W).  Around them
// 2 bytes of zlib header, the pad to a byte and 4 bytes of Adler-32.
MMH_HD int64_t enc_slot_bytes(int H, int W) {
    const int64_t raw = (int64_t)H * (1 + 3 * (int64_t)W), ns = enc_nseg(H);
    const int64_t bits = ns * (int64_t)(ENC_HDR_MAX_BITS + 9) + 9 * raw;
    return 2 + (bits + 7) / 8 + 4;
}
MMH_HD int64_t enc_meta_bytes(int N, int H) { return (int64_t)N * enc_nseg(H) * ENC_META_WORDS * 4; }
MMH_HD int64_t enc_scratch_bytes(int N, int H, int W) { return enc_meta_bytes(N, H) + (int64_t)N * H * (1 + 3 * (int64_t)W); }

struct HostEncLanes {
    static constexpr uint32_t N = 1;
    uint32_t lane() const { return 0; }
    void sync() const {}
    void add32(uint32_t* p, uint32_t v) const { *p += v; }
    void add64(uint64_t* p, uint64_t v) const { *p += v; }
    void or32(uint32_t* p, uint32_t v) const { *p |= v; }
};

template <uint32_t NL>
struct EncShared {
    uint64_t acc[8];                       // [0, 5): a row's filter sums; [5, 7): Adler terms; pass C: bit totals
    uint32_t hist[260];                    // literals 0 .. 255 and end-of-block
    uint32_t clhist[20];
    uint32_t lw[260], iw[260];             // leaf weights in ascending order; internal nodes' weights in creation order
    uint16_t order[260], lpar[260], ipar[260], idep[260];
    uint32_t code[260];                    // bit-reversed code | length << 16
    uint32_t clcode[20];
    uint32_t hdr[ENC_HDR_WORDS];
    uint32_t obuf[ENC_OBUF_WORDS];
    uint32_t scan[2][NL];
    uint32_t ntok, hdr_bits, flag;
    uint8_t len[260], cllen[20];
    uint8_t tok[260][2];                   // code-length symbol, extra-bits value
};

MMH_HD uint32_t enc_absb(uint32_t v) { return v < 128 ? v : 256 - v; }
MMH_HD uint32_t enc_paeth(int a, int b, int c) {
    int pa = b - c, pb = a - c, pc = a + b - 2 * c;
    pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}
MMH_HD uint32_t enc_filter(int ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : enc_paeth((int)a, (int)b, (int)c);
    return (x - pred) & 255;
}

// Code lengths of a complete prefix code over the symbols with freq > 0 (at least two: a lone or absent symbol gets company
// from symbol 0 or 1), none longer than maxlen; 0 for the others.  Huffman's lengths by the two-queue merge over the sorted
// weights; where the tree is deeper than maxlen the lengths are clamped and the histogram of lengths is repaired until its
// Kraft sum is exactly 1 (drop one maxlen code, split the deepest shorter one: the sum falls by 2^-maxlen per round), then
// the lengths are dealt out longest to the rarest.  A heuristic, not package-merge: enc_pass_a bounds it with the flat code.
template <class L, uint32_t NL>
MMH_HD void enc_build_lengths(L ln, EncShared<NL>& sh, uint32_t* freq, int nsym, int maxlen, uint8_t* out) {
    if (ln.lane() == 0) {
        int used = 0;
        for (int i = 0; i < nsym; ++i) used += freq[i] != 0;
        for (int i = 0; used < 2 && i < nsym; ++i)
            if (freq[i] == 0) { freq[i] = 1; ++used; }
        sh.flag = (uint32_t)used;
    }
    ln.sync();
    for (int i = ln.lane(); i < nsym; i += L::N) {            // rank sort by (frequency, symbol)
        out[i] = 0;
        const uint32_t f = freq[i];
        if (f == 0) continue;
        int r = 0;
        for (int j = 0; j < nsym; ++j) {
            const uint32_t g = freq[j];
            r += g != 0 && (g < f || (g == f && j < i));
        }
        sh.order[r] = (uint16_t)i;
        sh.lw[r] = f;
    }
    ln.sync();
    if (ln.lane() == 0) {
        const int n = (int)sh.flag;
        int i = 0, j = 0;
        for (int k = 0; k < n - 1; ++k) {
            uint32_t w = 0;
            for (int t = 0; t < 2; ++t) {
                if (i < n && (j >= k || sh.lw[i] <= sh.iw[j])) { w += sh.lw[i]; sh.lpar[i++] = (uint16_t)k; }
                else { w += sh.iw[j]; sh.ipar[j++] = (uint16_t)k; }
            }
            sh.iw[k] = w;
        }
        uint32_t cnt[17];
        for (int l = 0; l <= 16; ++l) cnt[l] = 0;
        sh.idep[n - 2] = 0;
        for (int k = n - 3; k >= 0; --k) sh.idep[k] = (uint16_t)(sh.idep[sh.ipar[k]] + 1);
        for (int k = 0; k < n; ++k) {
            const int d = sh.idep[sh.lpar[k]] + 1;
            ++cnt[d < maxlen ? d : maxlen];
        }
        uint32_t total = 0;
        for (int l = 1; l <= maxlen; ++l) total += cnt[l] << (maxlen - l);
        while (total > (1u << maxlen) && cnt[maxlen] > 0) {
            --cnt[maxlen];
            for (int l = maxlen - 1; l > 0; --l)
                if (cnt[l]) { --cnt[l]; cnt[l + 1] += 2; break; }
            --total;
        }
        int idx = 0;
        for (int l = maxlen; l >= 1; --l)
            for (uint32_t c = 0; c < cnt[l] && idx < n; ++c) out[sh.order[idx++]] = (uint8_t)l;
    }
    ln.sync();
}

// canonical codes (RFC 1951 3.2.2) of lens[0 .. nsym), bit-reversed for the LSB-first stream: code | length << 16.  One lane.
MMH_HD void enc_assign_codes(const uint8_t* lens, int nsym, uint32_t* out) {
    uint32_t cnt[16], next[16];
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < nsym; ++s) ++cnt[lens[s]];
    cnt[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (int s = 0; s < nsym; ++s) {
        const uint32_t l = lens[s];
        out[s] = l ? (bitrev(next[l]++, (int)l) | l << 16) : 0;
    }
}

struct EncBits {                                               // one lane's bit writer into a word array
    uint32_t* w;
    uint64_t acc;
    uint32_t n, wi, total;
    MMH_HD EncBits(uint32_t* w_) : w(w_), acc(0), n(0), wi(0), total(0) {}
    MMH_HD void put(uint32_t v, uint32_t bits) {
        acc |= (uint64_t)v << n;
        n += bits;
        total += bits;
        if (n >= 32) { w[wi++] = (uint32_t)acc; acc >>= 32; n -= 32; }
    }
    MMH_HD void finish() { if (n) w[wi] = (uint32_t)acc; }
};

// sh.len[0 .. 257) -> the dynamic block's header in sh.hdr / sh.hdr_bits: 257 literal / length codes, ONE distance code of
// length 1 (the form RFC 1951 3.2.7 gives for a block without matches), the 258 lengths run-length coded with 16 / 17 / 18
template <class L, uint32_t NL>
MMH_HD void enc_make_header(L ln, EncShared<NL>& sh, bool final) {
    if (ln.lane() == 0) {
        for (int i = 0; i < 19; ++i) sh.clhist[i] = 0;
        uint32_t nt = 0;
        auto emit = [&](uint32_t s, uint32_t extra) {
            sh.tok[nt][0] = (uint8_t)s;
            sh.tok[nt][1] = (uint8_t)extra;
            ++nt;
            ++sh.clhist[s];
        };
        auto at = [&](int i) -> uint32_t { return i < 257 ? sh.len[i] : 1; };
        for (int i = 0; i < 258;) {
            const uint32_t v = at(i);
            int run = 1;
            while (i + run < 258 && at(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int t = run < 138 ? run : 138; emit(18, (uint32_t)t - 11); run -= t; }
                if (run >= 3) { emit(17, (uint32_t)run - 3); run = 0; }
                while (run-- > 0) emit(0, 0);
            } else {
                emit(v, 0);
                --run;
                while (run >= 3) { const int t = run < 6 ? run : 6; emit(16, (uint32_t)t - 3); run -= t; }
                while (run-- > 0) emit(v, 0);
            }
        }
        sh.ntok = nt;
    }
    ln.sync();
    enc_build_lengths(ln, sh, sh.clhist, 19, 7, sh.cllen);
    if (ln.lane() == 0) {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        enc_assign_codes(sh.cllen, 19, sh.clcode);
        int hclen = 19;
        while (hclen > 4 && sh.cllen[order[hclen - 1]] == 0) --hclen;
        EncBits b(sh.hdr);
        b.put(final ? 1 : 0, 1);
        b.put(2, 2);
        b.put(0, 5);                                           // HLIT: 257 codes
        b.put(0, 5);                                           // HDIST: 1 code
        b.put((uint32_t)hclen - 4, 4);
        for (int i = 0; i < hclen; ++i) b.put(sh.cllen[order[i]], 3);
        for (uint32_t t = 0; t < sh.ntok; ++t) {
            const uint32_t s = sh.tok[t][0], c = sh.clcode[s];
            b.put(c & 0xffff, c >> 16);
            if (s >= 16) b.put(sh.tok[t][1], s == 16 ? 2 : s == 17 ? 3 : 7);
        }
        b.finish();
        sh.hdr_bits = b.total;
    }
    ln.sync();
}

// Pass A for segment `seg` of one image.  px: the image's pixels [H][W][3]; filt: the image's H (1 + 3 W) filtered bytes;
// meta: this segment's ENC_META_WORDS words.
template <class L, uint32_t NL>
MMH_HD void enc_pass_a(L ln, EncShared<NL>& sh, const uint8_t* px, int H, int W, int bgr, int64_t seg, int64_t nseg, uint8_t* filt,
                       uint32_t* meta) {
    const uint32_t lane = ln.lane();
    const int64_t stride = 1 + 3 * (int64_t)W;
    const int r0 = (int)(seg * ENC_SEG_ROWS), r1 = r0 + ENC_SEG_ROWS < H ? r0 + ENC_SEG_ROWS : H;
    const uint32_t nb = (uint32_t)((r1 - r0) * stride);
    uint8_t* sf = filt + r0 * stride;
    const int o0 = bgr ? 2 : 0, o2 = bgr ? 0 : 2;
    for (uint32_t i = lane; i < 260; i += L::N) sh.hist[i] = 0;
    for (uint32_t i = lane; i < 8; i += L::N) sh.acc[i] = 0;
    ln.sync();
    uint64_t ad_a = 0, ad_b = 0;
    for (int r = r0; r < r1; ++r) {
        const uint8_t* cur = px + (int64_t)r * W * 3;
        const uint8_t* up = r ? cur - (int64_t)W * 3 : nullptr;
        uint64_t s[5] = {0, 0, 0, 0, 0};
        for (int x = lane; x < W; x += L::N) {
            const int offs[3] = {o0, 1, o2};
            for (int c = 0; c < 3; ++c) {
                const int o = offs[c];
                const uint32_t v = cur[3 * x + o], a = x ? cur[3 * (x - 1) + o] : 0, b = up ? up[3 * x + o] : 0,
                               cc = (up && x) ? up[3 * (x - 1) + o] : 0;
                for (int ft = 0; ft < 5; ++ft) s[ft] += enc_absb(enc_filter(ft, v, a, b, cc));
            }
        }
        for (int ft = 0; ft < 5; ++ft)
            if (s[ft]) ln.add64(&sh.acc[ft], s[ft]);
        ln.sync();
        int best = 0;
        for (int ft = 1; ft < 5; ++ft)
            if (sh.acc[ft] < sh.acc[best]) best = ft;
        uint8_t* row = sf + (r - r0) * stride;
        const uint32_t base = (uint32_t)((r - r0) * stride);   // index of the filter byte inside the segment
        for (int x = lane; x < W; x += L::N) {
            const int offs[3] = {o0, 1, o2};
            for (int c = 0; c < 3; ++c) {
                const int o = offs[c];
                const uint32_t v = cur[3 * x + o], a = x ? cur[3 * (x - 1) + o] : 0, b = up ? up[3 * x + o] : 0,
                               cc = (up && x) ? up[3 * (x - 1) + o] : 0;
                const uint32_t f = enc_filter(best, v, a, b, cc);
                row[1 + 3 * x + c] = (uint8_t)f;
                ln.add32(&sh.hist[f], 1);
                ad_a += f;
                ad_b += (uint64_t)((nb - (base + 1 + 3 * (uint32_t)x + c)) % ADLER_P) * f;
            }
        }
        if (lane == 0) {
            row[0] = (uint8_t)best;
            ln.add32(&sh.hist[best], 1);
            ad_a += (uint32_t)best;
            ad_b += (uint64_t)((nb - base) % ADLER_P) * (uint32_t)best;
        }
        ln.sync();                                             // every lane has read this row's sums
        for (uint32_t i = lane; i < 5; i += L::N) sh.acc[i] = 0;
        ln.sync();
    }
    ln.add64(&sh.acc[5], ad_a % ADLER_P);
    ln.add64(&sh.acc[6], ad_b % ADLER_P);
    if (lane == 0) sh.hist[256] = 1;
    ln.sync();
    enc_build_lengths(ln, sh, sh.hist, 257, 15, sh.len);
    enc_make_header(ln, sh, seg == nseg - 1);
    if (lane == 0) {
        uint64_t data = 0;
        for (int s = 0; s < 257; ++s) data += (uint64_t)sh.hist[s] * sh.len[s];
        const uint64_t flat = 8ull * nb + sh.hist[255] + 9;
        sh.acc[7] = data + sh.hdr_bits;
        sh.flag = data + sh.hdr_bits > flat;                   // the flat code may be cheaper: cost its header too
    }
    ln.sync();
    if (sh.flag) {
        const uint64_t mine = sh.acc[7];
        ln.sync();
        for (uint32_t i = lane; i < 257; i += L::N) sh.len[i] = i < 255 ? 8 : 9;
        ln.sync();
        enc_make_header(ln, sh, seg == nseg - 1);
        const uint64_t flat = 8ull * nb + sh.hist[255] + 9 + sh.hdr_bits;
        if (flat >= mine) {                                    // the limited code wins after all: build it again
            ln.sync();
            enc_build_lengths(ln, sh, sh.hist, 257, 15, sh.len);
            enc_make_header(ln, sh, seg == nseg - 1);
        } else {
            ln.sync();
            if (lane == 0) sh.acc[7] = flat;
            ln.sync();
        }
    }
    if (lane == 0) enc_assign_codes(sh.len, 257, sh.code);
    ln.sync();
    for (uint32_t i = lane; i < ENC_HDR_WORDS; i += L::N) meta[EM_HDR + i] = i < (sh.hdr_bits + 31) / 32 ? sh.hdr[i] : 0;
    for (uint32_t i = lane; i < ENC_META_WORDS - EM_CODE; i += L::N) meta[EM_CODE + i] = i < 257 ? sh.code[i] : 0;
    if (lane == 0) {
        meta[EM_BITS_LO] = (uint32_t)sh.acc[7];
        meta[EM_BITS_HI] = (uint32_t)(sh.acc[7] >> 32);
        meta[EM_HDR_BITS] = sh.hdr_bits;
        meta[EM_ADLER_A] = (uint32_t)(sh.acc[5] % ADLER_P);
        meta[EM_ADLER_B] = (uint32_t)(sh.acc[6] % ADLER_P);
        meta[EM_NBYTES] = nb;
        meta[7] = 0;
        uint32_t tail = 0;
        if (seg != nseg - 1) {                                 // the block's last 7 bits: end-of-block and the literals before it
            uint32_t curb = sh.code[256] & 0xffff, nbit = sh.code[256] >> 16;
            for (int64_t k = (int64_t)nb - 1; nbit < 7 && k >= 0; --k) {
                const uint32_t c = sh.code[sf[k]];
                curb = (c & 0xffff) | curb << (c >> 16);
                nbit += c >> 16;
            }
            tail = nbit >= 7 ? (curb >> (nbit - 7)) & 127 : 0;
        }
        meta[EM_TAIL] = tail;
    }
}

template <class L, uint32_t NL>
MMH_HD uint32_t enc_excl_scan(L ln, EncShared<NL>& sh, uint32_t v, uint32_t& total) {
    const uint32_t lane = ln.lane();
    int src = 0;
    sh.scan[0][lane] = v;
    ln.sync();
    for (uint32_t o = 1; o < L::N; o <<= 1) {
        uint32_t x = sh.scan[src][lane];
        if (lane >= o) x += sh.scan[src][lane - o];
        sh.scan[src ^ 1][lane] = x;
        ln.sync();
        src ^= 1;
    }
    const uint32_t incl = sh.scan[src][lane];
    total = sh.scan[src][L::N - 1];
    ln.sync();
    return incl - v;
}

// Pass C for segment `seg` of one image.  filt / metas: the image's filtered rows and its nseg META blocks (pass A complete for
// all of them); slot: the image's slot_bytes output bytes.
template <class L, uint32_t NL>
MMH_HD void enc_pass_c(L ln, EncShared<NL>& sh, int H, int W, int64_t seg, int64_t nseg, const uint8_t* filt, const uint32_t* metas,
                       uint8_t* slot, int64_t slot_bytes, int64_t* length, int32_t* status) {
    const uint32_t lane = ln.lane();
    const int64_t stride = 1 + 3 * (int64_t)W;
    const uint32_t* meta = metas + seg * ENC_META_WORDS;
    if (lane == 0) sh.acc[0] = sh.acc[1] = 0;
    ln.sync();
    {
        uint64_t all = 0, before = 0;
        for (int64_t s = lane; s < nseg; s += L::N) {
            const uint64_t b = metas[s * ENC_META_WORDS + EM_BITS_LO] | (uint64_t)metas[s * ENC_META_WORDS + EM_BITS_HI] << 32;
            all += b;
            if (s < seg) before += b;
        }
        if (all) ln.add64(&sh.acc[0], all);
        if (before) ln.add64(&sh.acc[1], before);
    }
    ln.sync();
    const uint64_t total_bits = 16 + sh.acc[0], off_bits = 16 + sh.acc[1];
    const int64_t need = (int64_t)((total_bits + 7) / 8) + 4;
    const bool last = seg == nseg - 1;
    if (need > slot_bytes) {
        if (last && lane == 0) { *status = MMH_PNGENC_E_ROOM; *length = need; }
        return;
    }
    const uint32_t nb = meta[EM_NBYTES], hdr_bits = meta[EM_HDR_BITS];
    const uint8_t* sf = filt + seg * ENC_SEG_ROWS * stride;
    for (uint32_t i = lane; i < 257; i += L::N) sh.code[i] = meta[EM_CODE + i];
    for (uint32_t i = lane; i < ENC_OBUF_WORDS; i += L::N) sh.obuf[i] = 0;
    ln.sync();
    int64_t gbyte = (int64_t)(off_bits >> 3);
    uint32_t cbits = (uint32_t)(off_bits & 7);
    if (lane == 0) {
        if (seg == 0) { slot[0] = 0x78; slot[1] = 0x01; }      // 32 KiB window, no dictionary, FCHECK: 0x7801 = 31 * 991
        else if (cbits) sh.obuf[0] = meta[EM_TAIL - (int)ENC_META_WORDS] >> (7 - cbits);
    }
    ln.sync();
    const uint8_t* ob = reinterpret_cast<const uint8_t*>(sh.obuf);
    // store the complete bytes of obuf's first `pos` bits, keep the partial byte as the next round's first
    auto flush = [&](uint32_t pos) {
        const uint32_t nby = pos >> 3;
        for (uint32_t k = lane; k < nby; k += L::N)
            if (gbyte + k < slot_bytes) slot[gbyte + k] = ob[k];
        const uint32_t carry = ob[nby];
        ln.sync();
        for (uint32_t i = lane; i < (pos >> 5) + 2 && i < ENC_OBUF_WORDS; i += L::N) sh.obuf[i] = 0;
        ln.sync();
        if (lane == 0) sh.obuf[0] = carry;
        ln.sync();
        gbyte += nby;
        cbits = pos & 7;
    };
    for (uint32_t j = lane; j < (hdr_bits + 31) / 32; j += L::N) {
        const uint64_t v = (uint64_t)meta[EM_HDR + j] << cbits;
        if ((uint32_t)v) ln.or32(&sh.obuf[j], (uint32_t)v);
        if (v >> 32) ln.or32(&sh.obuf[j + 1], (uint32_t)(v >> 32));
    }
    ln.sync();
    flush(cbits + hdr_bits);
    const uint32_t nsym = nb + 1;                              // the literals and end-of-block
    constexpr uint32_t SPL = ENC_TILE / L::N;
    for (uint32_t t0 = 0; t0 < nsym; t0 += ENC_TILE) {
        const uint32_t first = t0 + lane * SPL;
        const uint32_t cnt = first >= nsym ? 0 : (nsym - first < SPL ? nsym - first : SPL);
        uint32_t lb = 0;
        for (uint32_t k = 0; k < cnt; ++k) lb += sh.code[first + k < nb ? sf[first + k] : 256] >> 16;
        uint32_t tile_bits;
        const uint32_t p = cbits + enc_excl_scan(ln, sh, lb, tile_bits);
        uint32_t wi = p >> 5, n = p & 31;
        uint64_t acc = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t c = sh.code[first + k < nb ? sf[first + k] : 256];
            acc |= (uint64_t)(c & 0xffff) << n;
            n += c >> 16;
            if (n >= 32) {
                if ((uint32_t)acc) ln.or32(&sh.obuf[wi], (uint32_t)acc);
                ++wi;
                acc >>= 32;
                n -= 32;
            }
        }
        if (n && (uint32_t)acc) ln.or32(&sh.obuf[wi], (uint32_t)acc);
        ln.sync();
        flush(cbits + tile_bits);
    }
    if (last && lane == 0) {
        if (cbits) {                                           // the pad to a byte
            if (gbyte < slot_bytes) slot[gbyte] = ob[0];
            ++gbyte;
        }
        uint64_t a = 1, b = 0;                                 // Adler-32 of the concatenation, segment by segment
        for (int64_t s = 0; s < nseg; ++s) {
            const uint32_t* m = metas + s * ENC_META_WORDS;
            b = (b + (uint64_t)(m[EM_NBYTES] % ADLER_P) * a + m[EM_ADLER_B]) % ADLER_P;
            a = (a + m[EM_ADLER_A]) % ADLER_P;
        }
        const uint32_t adler = (uint32_t)(b << 16 | a);
        for (int k = 0; k < 4; ++k)
            if (gbyte + k < slot_bytes) slot[gbyte + k] = (uint8_t)(adler >> (24 - 8 * k));
        *length = gbyte + 4;
        *status = MMH_PNGENC_OK;
    }
}

}  // namespace mmh_png

// The bit-level core of the PNG decoder (png_decode.hip on the device, png_host.cpp on the host): zlib / DEFLATE
// (RFC 1950 / 1951) into a 32 KiB sliding window that is flushed to the image's scratch slot in 8 KiB pieces, with the
// Adler-32 of the flushed bytes.  ONE implementation for both builds: the code is written for `L::N` lanes that run it in
// lockstep - every lane decodes the same symbols from the same staged input (symbol decode is wave-uniform), and the three
// cooperative parts (input refill, match copy, window flush) are lane-strided loops.  The host build runs it with one lane,
// so every index computation and every bounds test the device executes is the one the CPU tests (and the ASan / UBSan
// variant, `make png_host_asan`) exercise.
//
// Bounds, by construction: the stream is read only inside [nxt, end) of refill(); the window is indexed `& WMASK`; the
// scratch slot is written only at [flushed, flushed + n) with flushed + n <= op <= total; every loop consumes input bits or
// produces output bytes, and `steps` (one per block, code length, symbol and stored piece) is capped by max_steps().
#pragma once
#include <stdint.h>

#include "../../include/mmhand_hip.h"

#if defined(__HIPCC__)
#define MMH_HD __host__ __device__ __forceinline__
#else
#define MMH_HD inline
#endif

namespace mmh_png {

constexpr uint32_t WIN = 32768, WMASK = WIN - 1;   // DEFLATE's largest window; the ring is exactly the window
constexpr uint32_t FLUSH = 8192;                   // flush piece (divides WIN: a piece never wraps)
constexpr uint32_t INBUF = 4096;                   // staged compressed bytes
constexpr int FAST_LIT = 10, FAST_DIST = 8;        // first-level lookup widths
constexpr uint32_t ADLER_P = 65521;

// what the window, the staged input and the Huffman tables take: LDS on the device (40.4 KiB: three images per CU)
struct Shared {
    alignas(16) uint8_t win[WIN];
    alignas(16) uint8_t inbuf[INBUF];
    uint16_t lit_fast[1 << FAST_LIT];     // (len << 9) | symbol for codes of <= FAST_LIT bits, 0 = take the canonical walk
    uint16_t dist_fast[1 << FAST_DIST];
    uint16_t lit_cnt[16], dist_cnt[16];   // codes per length
    uint16_t lit_sym[288], dist_sym[32];  // symbols in canonical order
    uint16_t offs[16];
    uint8_t lens[352];                    // [0, 32): code-length code or the fixed set's head; dynamic lengths from 32
};

// every inflate loop iteration counts one step; none can run without consuming at least one input bit, except the (at most
// 8 + out / 1) stored pieces and flushes that produce output instead
MMH_HD uint64_t max_steps(uint64_t in_bytes, uint64_t out_bytes) { return 8 * in_bytes + out_bytes + 64; }

// length symbol 257 + s -> base and extra bits; distance symbol d -> base and extra bits (RFC 1951 3.2.5, in closed form)
MMH_HD void length_code(uint32_t s, uint32_t& base, uint32_t& extra) {
    if (s < 8) { base = 3 + s; extra = 0; }
    else if (s == 28) { base = 258; extra = 0; }
    else { extra = (s - 4) >> 2; base = 3 + ((4 + (s & 3)) << extra); }
}
MMH_HD void dist_code(uint32_t d, uint32_t& base, uint32_t& extra) {
    if (d < 4) { base = 1 + d; extra = 0; }
    else { extra = (d >> 1) - 1; base = 1 + ((2 + (d & 1)) << extra); }
}
MMH_HD uint32_t bitrev(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

struct HostLanes {
    static constexpr uint32_t N = 1;
    uint32_t lane() const { return 0; }
    void sync() const {}
    uint32_t sum(uint32_t v) const { return v; }
};

struct alignas(16) V16 { uint32_t x[4]; };

template <class L>
struct Inflater {
    L ln;
    Shared& sh;
    const uint8_t* src;       // the batch's stream buffer
    int64_t nxt, end;         // this image's unread range of it
    uint32_t pos, lim;        // unread range of sh.inbuf
    uint64_t bitbuf;
    uint32_t bitcnt;
    uint8_t* dst;             // this image's scratch slot, `total` bytes
    uint32_t op, total, flushed;
    uint32_t ad_a, ad_b;
    uint64_t steps, step_cap;

    MMH_HD Inflater(L l, Shared& s, const uint8_t* src_, int64_t beg, int64_t end_, uint8_t* dst_, uint32_t total_)
        : ln(l), sh(s), src(src_), nxt(beg), end(end_), pos(0), lim(0), bitbuf(0), bitcnt(0), dst(dst_), op(0),
          total(total_), flushed(0), ad_a(1), ad_b(0), steps(0),
          step_cap(max_steps((uint64_t)(end_ - beg), total_)) {}

    // ---- cooperative: stage the next <= INBUF bytes of the stream; aligned dwords where the whole dword is the image's
    MMH_HD bool refill() {
        if (nxt >= end) return false;
        ln.sync();
        const uintptr_t g = (uintptr_t)src + (uintptr_t)nxt;
        const uint32_t a = (uint32_t)(g & 3);
        const int64_t left = end - nxt;
        const uint32_t n = left < (int64_t)(INBUF - a) ? (uint32_t)left : INBUF - a;
        const uintptr_t g0 = g - a;                       // inbuf[k] <-> byte g0 + k, k in [a, a + n)
        const uint32_t ndw = (a + n + 3) >> 2;
        uint32_t* in32 = reinterpret_cast<uint32_t*>(sh.inbuf);
        for (uint32_t j = ln.lane(); j < ndw; j += L::N) {
            const uint32_t lo = 4 * j;
            uint32_t v = 0;
            if (lo >= a && lo + 4 <= a + n) {
                v = *reinterpret_cast<const uint32_t*>(g0 + lo);
            } else {
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t k = lo + b;
                    if (k >= a && k < a + n) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(g0 + k) << (8 * b);
                }
            }
            in32[j] = v;
        }
        pos = a;
        lim = a + n;
        nxt += n;
        ln.sync();
        return true;
    }

    // ---- bit reader: after fill() more than 32 bits are buffered unless the stream has ended
    MMH_HD void fill() {
        while (bitcnt <= 32) {
            if (pos == lim && !refill()) return;
            if ((pos & 3) == 0 && pos + 4 <= lim) {
                bitbuf |= (uint64_t)*reinterpret_cast<const uint32_t*>(sh.inbuf + pos) << bitcnt;
                bitcnt += 32;
                pos += 4;
            } else {
                bitbuf |= (uint64_t)sh.inbuf[pos++] << bitcnt;
                bitcnt += 8;
            }
        }
    }
    MMH_HD void drop(uint32_t n) { bitbuf >>= n; bitcnt -= n; }
    // n <= 16; false = the stream ended first
    MMH_HD bool bits(uint32_t n, uint32_t& v) {
        fill();
        if (bitcnt < n) return false;
        v = (uint32_t)bitbuf & ((1u << n) - 1);
        drop(n);
        return true;
    }

    // ---- cooperative: window -> scratch, with the piece's Adler-32 sums
    MMH_HD void flush_piece(uint32_t n) {
        ln.sync();
        const uint8_t* w = sh.win + (flushed & WMASK);
        uint8_t* d = dst + flushed;
        uint32_t s1 = 0;                                  // sum d_j, sum j d_j over this lane's bytes of the piece
        uint64_t s2 = 0;
        uint32_t done = 0;
        if (((uintptr_t)d & 15) == 0) {
            const uint32_t nv = n >> 4;
            for (uint32_t g = ln.lane(); g < nv; g += L::N) {
                const V16 v = *reinterpret_cast<const V16*>(w + 16 * g);
                *reinterpret_cast<V16*>(d + 16 * g) = v;
                for (uint32_t q = 0; q < 4; ++q)
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint32_t x = (v.x[q] >> (8 * b)) & 255;
                        s1 += x;
                        s2 += (uint64_t)(16 * g + 4 * q + b) * x;
                    }
            }
            done = nv << 4;
        }
        for (uint32_t j = done + ln.lane(); j < n; j += L::N) {
            const uint32_t x = w[j];
            d[j] = (uint8_t)x;
            s1 += x;
            s2 += (uint64_t)j * x;
        }
        const uint32_t t1 = ln.sum(s1), t2 = ln.sum((uint32_t)(s2 % ADLER_P));
        ad_b = (uint32_t)(((uint64_t)ad_b + (uint64_t)n * ad_a + (uint64_t)n * t1 + (uint64_t)ADLER_P * L::N - t2) % ADLER_P);
        ad_a = (ad_a + t1) % ADLER_P;
        flushed += n;
        ln.sync();
    }
    MMH_HD void produced(uint32_t n) {
        op += n;
        while (op - flushed >= FLUSH) flush_piece(FLUSH);
    }
    MMH_HD void literal(uint32_t b) {
        if (ln.lane() == 0) sh.win[op & WMASK] = (uint8_t)b;
        produced(1);
    }
    // ---- cooperative: copy `len` bytes from `dist` back; byte i of an overlapping copy repeats the period it started with
    MMH_HD void match(uint32_t dist, uint32_t len) {
        ln.sync();
        for (uint32_t i = ln.lane(); i < len; i += L::N) {
            const uint32_t k = i < dist ? i : i % dist;
            sh.win[(op + i) & WMASK] = sh.win[(op - dist + k) & WMASK];
        }
        ln.sync();
        produced(len);
    }
    // ---- cooperative: n staged input bytes -> window (a stored block); n <= lim - pos and n <= FLUSH - (op - flushed)
    MMH_HD void stored(uint32_t n) {
        ln.sync();
        for (uint32_t i = ln.lane(); i < n; i += L::N) sh.win[(op + i) & WMASK] = sh.inbuf[pos + i];
        ln.sync();
        pos += n;
        produced(n);
    }

    // ---- canonical Huffman tables (the construction of zlib's puff.c, plus a first-level lookup).  Returns 0, or
    // MMH_PNG_E_CODE_OVER / MMH_PNG_E_CODE_INCOMPLETE.  An incomplete set is accepted only when its longest code has one
    // bit (zlib's rule: the single-distance-code streams old deflaters wrote); its unassigned pattern decodes to an error.
    MMH_HD int build(const uint8_t* lens, uint32_t n, uint16_t* cnt, uint16_t* sym, uint16_t* fast, int fastbits) {
        ln.sync();
        for (uint32_t j = ln.lane(); j < (1u << fastbits); j += L::N) fast[j] = 0;
        if (ln.lane() == 0) {
            for (int l = 0; l < 16; ++l) cnt[l] = 0;
            for (uint32_t s = 0; s < n; ++s) cnt[lens[s]]++;
        }
        ln.sync();
        int left = 1, maxlen = 0;
        for (int l = 1; l < 16; ++l) {
            left = (left << 1) - (int)cnt[l];
            if (left < 0) return MMH_PNG_E_CODE_OVER;
            if (cnt[l]) maxlen = l;
        }
        if (left > 0 && maxlen > 1) return MMH_PNG_E_CODE_INCOMPLETE;
        if (ln.lane() == 0) {
            sh.offs[1] = 0;
            for (int l = 1; l < 15; ++l) sh.offs[l + 1] = sh.offs[l] + cnt[l];
            for (uint32_t s = 0; s < n; ++s)
                if (lens[s]) sym[sh.offs[lens[s]]++] = (uint16_t)s;
        }
        ln.sync();
        uint32_t code = 0, idx = 0;
        for (int l = 1; l <= fastbits; ++l) {
            for (uint32_t k = 0; k < cnt[l]; ++k, ++code, ++idx) {
                const uint16_t e = (uint16_t)((l << 9) | sym[idx]);
                for (uint32_t j = bitrev(code, l) + (ln.lane() << l); j < (1u << fastbits); j += L::N << l) fast[j] = e;
            }
            code <<= 1;
        }
        ln.sync();
        return 0;
    }
    // one symbol; < 0: -(status)
    MMH_HD int decode(const uint16_t* cnt, const uint16_t* sym, const uint16_t* fast, int fastbits) {
        fill();
        const uint32_t e = fast[(uint32_t)bitbuf & ((1u << fastbits) - 1)];
        if (e) {
            const uint32_t l = e >> 9;
            if (l > bitcnt) return -MMH_PNG_E_TRUNCATED;
            drop(l);
            return (int)(e & 511);
        }
        uint32_t b = (uint32_t)bitbuf;
        int code = 0, first = 0, index = 0;
        for (uint32_t l = 1; l <= 15; ++l) {
            code |= (int)(b & 1);
            b >>= 1;
            const int count = cnt[l];
            if (code - count < first) {
                if (l > bitcnt) return -MMH_PNG_E_TRUNCATED;
                drop(l);
                return sym[index + (code - first)];
            }
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
        return bitcnt < 15 ? -MMH_PNG_E_TRUNCATED : -MMH_PNG_E_BAD_CODE;
    }

    MMH_HD int dynamic_tables() {
        uint32_t hl, hd, hc, v;
        if (!bits(5, hl) || !bits(5, hd) || !bits(4, hc)) return MMH_PNG_E_TRUNCATED;
        const uint32_t nlen = hl + 257, ndist = hd + 1, ncode = hc + 4;
        if (nlen > 286 || ndist > 30) return MMH_PNG_E_CODE_COUNT;
        // the order of the code-length code lengths, 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
        const uint64_t o0 = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                            10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
        const uint64_t o1 = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        uint32_t cl[19];
        for (uint32_t i = 0; i < 19; ++i) {
            uint32_t len = 0;
            if (i < ncode) {
                if (!bits(3, len)) return MMH_PNG_E_TRUNCATED;
            }
            cl[i] = len;
        }
        ln.sync();
        if (ln.lane() == 0)
            for (uint32_t i = 0; i < 19; ++i) sh.lens[(uint32_t)((i < 12 ? o0 >> (5 * i) : o1 >> (5 * (i - 12))) & 31)] = (uint8_t)cl[i];
        ln.sync();
        // the code-length code decodes through the literal tables' storage; it must be complete (zlib)
        int rc = build(sh.lens, 19, sh.lit_cnt, sh.lit_sym, sh.lit_fast, 7);
        if (rc) return rc;
        {
            int left = 1;
            for (int l = 1; l < 16; ++l) left = (left << 1) - (int)sh.lit_cnt[l];
            if (left > 0) return MMH_PNG_E_CODE_INCOMPLETE;
        }
        // lengths go to lens[32 ..]: lens[0 .. 18] still feed the table just built only through cnt / sym, not lens
        uint8_t* out = sh.lens + 32;
        uint32_t i = 0, prev = 0;
        while (i < nlen + ndist) {
            if (++steps > step_cap) return MMH_PNG_E_STEPS;
            const int s = decode(sh.lit_cnt, sh.lit_sym, sh.lit_fast, 7);
            if (s < 0) return -s;
            if (s < 16) {
                if (ln.lane() == 0) out[i] = (uint8_t)s;
                prev = (uint32_t)s;
                ++i;
                continue;
            }
            uint32_t rep, val = 0;
            if (s == 16) {
                if (i == 0) return MMH_PNG_E_REPEAT;
                if (!bits(2, v)) return MMH_PNG_E_TRUNCATED;
                rep = 3 + v;
                val = prev;
            } else if (s == 17) {
                if (!bits(3, v)) return MMH_PNG_E_TRUNCATED;
                rep = 3 + v;
            } else {
                if (!bits(7, v)) return MMH_PNG_E_TRUNCATED;
                rep = 11 + v;
            }
            if (i + rep > nlen + ndist) return MMH_PNG_E_CODE_COUNT;
            if (ln.lane() == 0)
                for (uint32_t k = 0; k < rep; ++k) out[i + k] = (uint8_t)val;
            i += rep;
            prev = val;
        }
        ln.sync();
        if (out[256] == 0) return MMH_PNG_E_NO_EOB;
        rc = build(out, nlen, sh.lit_cnt, sh.lit_sym, sh.lit_fast, FAST_LIT);
        if (rc) return rc;
        return build(out + nlen, ndist, sh.dist_cnt, sh.dist_sym, sh.dist_fast, FAST_DIST);
    }
    MMH_HD int fixed_tables() {
        ln.sync();
        for (uint32_t s = ln.lane(); s < 320; s += L::N)
            sh.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        ln.sync();
        int rc = build(sh.lens, 288, sh.lit_cnt, sh.lit_sym, sh.lit_fast, FAST_LIT);
        if (rc) return rc;
        return build(sh.lens + 288, 32, sh.dist_cnt, sh.dist_sym, sh.dist_fast, FAST_DIST);   // 30 and 31 have codes too
    }

    MMH_HD int stored_block() {
        uint32_t len, nlen;
        drop(bitcnt & 7);
        if (!bits(16, len) || !bits(16, nlen)) return MMH_PNG_E_TRUNCATED;
        if ((len ^ 0xffffu) != nlen) return MMH_PNG_E_STORED_LEN;
        if (len > total - op) return MMH_PNG_E_OUTPUT_LONG;
        while (len) {
            if (++steps > step_cap) return MMH_PNG_E_STEPS;
            if (bitcnt) {                                  // whole bytes the bit reader had taken already
                literal((uint32_t)bitbuf & 255);
                drop(8);
                --len;
                continue;
            }
            if (pos == lim && !refill()) return MMH_PNG_E_TRUNCATED;
            uint32_t n = len < lim - pos ? len : lim - pos;
            const uint32_t room = FLUSH - (op - flushed);
            if (n > room) n = room;
            stored(n);
            len -= n;
        }
        return 0;
    }

    MMH_HD int codes_block() {
        for (;;) {
            if (++steps > step_cap) return MMH_PNG_E_STEPS;
            int s = decode(sh.lit_cnt, sh.lit_sym, sh.lit_fast, FAST_LIT);
            if (s < 0) return -s;
            if (s < 256) {
                if (op >= total) return MMH_PNG_E_OUTPUT_LONG;
                literal((uint32_t)s);
                continue;
            }
            if (s == 256) return 0;
            if (s > 285) return MMH_PNG_E_SYMBOL;
            uint32_t base, extra, v = 0;
            length_code((uint32_t)s - 257, base, extra);
            if (extra && !bits(extra, v)) return MMH_PNG_E_TRUNCATED;
            const uint32_t len = base + v;
            s = decode(sh.dist_cnt, sh.dist_sym, sh.dist_fast, FAST_DIST);
            if (s < 0) return -s;
            if (s > 29) return MMH_PNG_E_SYMBOL;
            dist_code((uint32_t)s, base, extra);
            v = 0;
            if (extra && !bits(extra, v)) return MMH_PNG_E_TRUNCATED;
            const uint32_t dist = base + v;
            if (dist > op) return MMH_PNG_E_DISTANCE;
            if (len > total - op) return MMH_PNG_E_OUTPUT_LONG;
            match(dist, len);
        }
    }

    // the whole stream; 0 = `total` bytes are in the scratch slot and their Adler-32 matches the trailer
    MMH_HD int run() {
        uint32_t cmf, flg, v;
        if (!bits(8, cmf) || !bits(8, flg)) return MMH_PNG_E_TRUNCATED;
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0) return MMH_PNG_E_HEADER;
        if (flg & 32) return MMH_PNG_E_DICT;
        uint32_t last;
        do {
            uint32_t type;
            if (++steps > step_cap) return MMH_PNG_E_STEPS;
            if (!bits(1, last) || !bits(2, type)) return MMH_PNG_E_TRUNCATED;
            int rc;
            if (type == 0) rc = stored_block();
            else if (type == 3) rc = MMH_PNG_E_BLOCK_TYPE;
            else {
                rc = type == 1 ? fixed_tables() : dynamic_tables();
                if (!rc) rc = codes_block();
            }
            if (rc) return rc;
        } while (!last);
        if (op != total) return MMH_PNG_E_OUTPUT_SHORT;
        drop(bitcnt & 7);
        uint32_t want = 0;
        for (int i = 0; i < 4; ++i) {
            if (!bits(8, v)) return MMH_PNG_E_TRUNCATED;
            want = (want << 8) | v;
        }
        fill();
        if (bitcnt) return MMH_PNG_E_TRAILING;
        if (op > flushed) flush_piece(op - flushed);
        if (((ad_b << 16) | ad_a) != want) return MMH_PNG_E_ADLER;
        return 0;
    }
};

MMH_HD uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p;
    const int pb = p > (int)b ? p - (int)b : (int)b - p;
    const int pc = p > (int)c ? p - (int)c : (int)c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// one reconstructed byte: x = filtered byte, a = left, b = up, c = up-left (PNG 9.2); ft <= 4
MMH_HD uint32_t unfilter_byte(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t add = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    return (x + add) & 255;
}

}  // namespace mmh_png

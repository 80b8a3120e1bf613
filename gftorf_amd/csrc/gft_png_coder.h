// gft_png_coder.h -- the segment coder of the PNG encoder (include/gftorf_png.h states the stream it writes), as the steps of
// one workgroup of PNG_THREADS threads over one segment of the filtered stream.  Every step is a function of (the workgroup's
// LDS, the segment, the thread's index) and the steps are separated by barriers, nothing else: k_png.hip calls them with
// __syncthreads() between, and a host program can call them for tid = 0 .. PNG_THREADS - 1 in turn (tests/test_png_host.py
// builds one with the address sanitizer and compares it with the numpy model, tests/png_ref.py).  What a thread keeps from
// one step to the next therefore lies in LDS, not in registers.
//
// LDS: `m` holds one 16-bit word per byte of the segment (a literal's byte; 0x8000 | candidate << 8 | length - 3 for a match at
// one of the five fixed distances; 0xc000 | length - 4 << 12 | bucket for a match at the bucket's first position); `htab` holds
// per bucket of the 4-byte hash the least position that falls into it (an LDS atomic min: the same in any order); `b` is
// used three times over: the filtered bytes while the matches are found, then the greedy parse's exit table (for every byte,
// where a parse that stands on it first leaves the thread's 128 bytes), then the chunk's bytes as they go to the scratch.
// A thread owns PNG_OWN = 128 consecutive bytes in the serial steps; `m`, the filtered bytes and the exit table are padded by
// one dword per 128 bytes, so that the threads of a wave, all at the same place of their own bytes, fall on different banks.
#pragma once
#include <stdint.h>
#include "gftorf_png.h"

#ifdef __HIPCC__
#define PNG_HD __host__ __device__ __forceinline__
#else
#define PNG_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_OR(word, bits) atomicOr((word), (bits))
#define PNG_MIN(word, value) atomicMin((word), (value))
#else
#define PNG_OR(word, bits) (*(word) |= (bits))
#define PNG_MIN(word, value) (*(word) = *(word) < (value) ? *(word) : (value))
#endif

constexpr int PNG_THREADS = 256;
constexpr int PNG_SEG = GFT_PNG_SEGMENT;
constexpr int PNG_OWN = PNG_SEG / PNG_THREADS;          // 128 bytes per thread
constexpr int PNG_OWN_SHIFT = 7;
constexpr int PNG_CANDIDATES = 5;                       // the fixed distances
constexpr int PNG_HASH_BITS = GFT_PNG_HASH_BITS, PNG_HASH_MIN = 4, PNG_HASH_MAX = 7;    // the hash candidate: buckets, lengths
constexpr uint32_t PNG_NONE = 0xffffu;
constexpr uint32_t PNG_ADLER = 65521u;
constexpr uint32_t PNG_POLY = 0xedb88320u;
constexpr int PNG_PIECE = 256;                          // bytes of a thread's CRC piece
constexpr int PNG_GROUP = 16;                           // pieces folded by one thread in the first CRC fold
static_assert(PNG_OWN == (1 << PNG_OWN_SHIFT) && PNG_THREADS * PNG_PIECE >= GFT_PNG_CHUNK_SLOT, "png coder layout");

struct PngLds {
    uint16_t m[PNG_SEG + 2 * PNG_THREADS];
    uint32_t b[(2 * PNG_SEG + 4 * PNG_THREADS + 64) / 4];
    uint16_t lead[PNG_CANDIDATES][PNG_THREADS];
    uint16_t entry[PNG_THREADS];
    uint32_t htab[1 << PNG_HASH_BITS];
    uint32_t crc_table[256];
    uint32_t red[PNG_THREADS];
    uint32_t red2[PNG_THREADS];
    uint32_t total_bits, adler_a, adler_b;
};

// one segment, the same in every thread
struct PngSeg {
    const uint8_t* src;        // the image
    const uint8_t* ftype;      // the image's filter type per row, nullptr: all 0
    int64_t stride;
    int32_t H, L, C;           // L = 1 + W * C
    uint32_t p0;               // the segment's first byte in the image's filtered stream
    int32_t n;                 // its bytes, 1 .. PNG_SEG
    int32_t first;             // the image's first segment: the zlib header goes in front
    int32_t level;
    uint32_t ldist_code, ldist_bits;   // the distance L as it goes into the bit stream: code with its extra bits, their count
    uint32_t x2n_piece, x2n_group;     // x^(8 * PNG_PIECE) and x^(8 * PNG_PIECE * PNG_GROUP) mod the CRC polynomial
};

PNG_HD int png_ix16(int p) { return p + ((p >> PNG_OWN_SHIFT) << 1); }      // index of a 16-bit entry
PNG_HD int png_ix8(int p) { return p + ((p >> PNG_OWN_SHIFT) << 2); }       // index of a filtered byte
PNG_HD int png_own(const PngSeg& s, int tid) { const int r = s.n - tid * PNG_OWN; return r < 0 ? 0 : (r > PNG_OWN ? PNG_OWN : r); }

// byte `col` of scanline `row` of the filtered stream
PNG_HD uint32_t png_filtered(const uint8_t* src, int64_t stride, int C, const uint8_t* ftype, uint32_t row, uint32_t col)
{
    const uint32_t t = ftype ? ftype[row] : 0u;
    if (col == 0) return t;
    const uint32_t x = col - 1;
    const uint8_t* r = src + (int64_t)row * stride;
    uint32_t v = r[x];
    if (t == 1) v -= x >= (uint32_t)C ? r[x - C] : 0u;
    else if (t == 2) v -= row > 0 ? (r - stride)[x] : 0u;
    return v & 255u;
}

PNG_HD uint32_t png_filtered_at(const PngSeg& s, int p)
{
    const uint32_t gp = s.p0 + (uint32_t)p, row = gp / (uint32_t)s.L;
    return png_filtered(s.src, s.stride, s.C, s.ftype, row, gp - row * (uint32_t)s.L);
}

PNG_HD int png_distance(const PngSeg& s, int q) { return q < 4 ? q + 1 : s.L; }

// the bucket of the four bytes g (the first byte lowest)
PNG_HD uint32_t png_bucket(uint32_t g) { return (g * 2654435761u) >> (32 - PNG_HASH_BITS); }

// the distance d (1 .. 32768) as deflate codes it: the 5-bit code most significant bit first, then the extra bits
PNG_HD uint32_t png_distance_bits(uint32_t d, uint32_t* nbits)
{
    uint32_t sym, extra = 0, ebits = 0;
    if (d <= 4) sym = d - 1;
    else {
        uint32_t top = 31;
        while (!(((d - 1) >> top) & 1u)) top--;
        ebits = top - 1;
        sym = 2 * top + (((d - 1) >> ebits) & 1u);
        extra = (d - 1) & ((1u << ebits) - 1u);
    }
    uint32_t rev = 0;
    for (int k = 0; k < 5; k++) rev |= ((sym >> k) & 1u) << (4 - k);
    *nbits = 5 + ebits;
    return rev | (extra << 5);
}

// a * b mod the CRC-32 polynomial, both reflected (bit 31 is x^0)
PNG_HD uint32_t png_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return p;
}

PNG_HD uint32_t png_crc_byte(uint32_t c, uint32_t byte)
{
    c ^= byte;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
    return c;
}

// the token of the 16-bit entry mm at byte j: its bits as they enter the stream from bit 0 up, and how many; at most 31
PNG_HD uint32_t png_token(const PngLds& lds, const PngSeg& s, uint32_t mm, int j, int* nbits)
{
    uint32_t sym, extra = 0, ebits = 0;
    if (!(mm & 0x8000u)) {
        sym = mm & 255u;
    } else if (mm & 0x4000u) {
        sym = 258 + ((mm >> 12) & 3u);                  // lengths 4 .. 7
    } else {
        const uint32_t l = mm & 255u;                   // length - 3
        if (l == 255u) sym = 285;
        else if (l < 8u) sym = 257 + l;
        else {
            uint32_t top = 31;
            while (!((l >> top) & 1u)) top--;
            ebits = top - 2;
            sym = 261 + 4 * ebits + ((l >> ebits) & 3u);
            extra = l & ((1u << ebits) - 1u);
        }
    }
    uint32_t code, len;
    if (sym < 144) { code = 0x30 + sym; len = 8; }
    else if (sym < 256) { code = 0x190 + (sym - 144); len = 9; }
    else if (sym < 280) { code = sym - 256; len = 7; }
    else { code = 0xc0 + (sym - 280); len = 8; }
    uint32_t rev = 0;
    for (uint32_t k = 0; k < len; k++) rev |= ((code >> k) & 1u) << (len - 1 - k);
    uint32_t bits = rev | (extra << len);
    int n = (int)(len + ebits);
    if ((mm & 0xc000u) == 0xc000u) {
        uint32_t dbits;
        const uint32_t dcode = png_distance_bits((uint32_t)j - lds.htab[mm & ((1u << PNG_HASH_BITS) - 1u)], &dbits);
        bits |= dcode << n;
        n += (int)dbits;
    } else if (mm & 0x8000u) {
        const uint32_t q = (mm >> 8) & 7u;
        if (q < 4) {                                    // distance codes 0..3: five bits, most significant first, no extra
            const uint32_t r5 = ((q & 1u) << 4) | ((q & 2u) << 2);
            bits |= r5 << n;
            n += 5;
        } else {
            bits |= s.ldist_code << n;
            n += (int)s.ldist_bits;
        }
    }
    *nbits = n;
    return bits;
}

PNG_HD int png_next(int j, uint32_t mm)
{
    if (!(mm & 0x8000u)) return j + 1;
    return j + ((mm & 0x4000u) ? PNG_HASH_MIN + (int)((mm >> 12) & 3u) : (int)(mm & 255u) + 3);
}

PNG_HD void png_or_byte(uint32_t* b, int pos, uint32_t v) { PNG_OR(&b[pos >> 2], v << (8 * (pos & 3))); }

PNG_HD void png_or_bits(uint32_t* b, uint32_t bitpos, uint32_t bits)
{
    const uint64_t v = (uint64_t)bits << (bitpos & 31u);
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (lo) PNG_OR(&b[bitpos >> 5], lo);
    if (hi) PNG_OR(&b[(bitpos >> 5) + 1], hi);
}

// what the chunk looks like once the token bits are counted (the same in every thread)
struct PngForm {
    int hdr;            // 2 in the image's first chunk
    int fixed;          // the fixed form is taken
    int data_bytes;     // the chunk's data
    int chunk_bytes;    // 12 + data_bytes
    uint32_t bits;      // of the fixed block with its end-of-block code and the empty stored block's header
};

PNG_HD PngForm png_form(const PngSeg& s, uint32_t token_bits)
{
    PngForm f;
    f.hdr = s.first ? 2 : 0;
    f.bits = 3u + token_bits + 10u;
    const int fixed_bytes = (int)((f.bits + 7u) >> 3) + 4, stored_bytes = 5 + s.n;
    f.fixed = s.level >= 1 && fixed_bytes <= stored_bytes;
    f.data_bytes = f.hdr + (f.fixed ? fixed_bytes : stored_bytes);
    f.chunk_bytes = 12 + f.data_bytes;
    return f;
}

// ---- the steps ------------------------------------------------------------------------------------------------------------

// 0: the CRC table, the filtered bytes into b, the thread's share of the Adler sums
PNG_HD void png_step_load(PngLds& l, const PngSeg& s, int tid)
{
    uint32_t c = (uint32_t)tid;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
    l.crc_table[tid] = c;
    l.entry[tid] = (uint16_t)PNG_NONE;
    for (int k = tid; k < (1 << PNG_HASH_BITS); k += PNG_THREADS) l.htab[k] = 0xffffffffu;
    uint8_t* f = reinterpret_cast<uint8_t*>(l.b);
    uint32_t A = 0, B = 0;
    for (int p = tid; p < s.n; p += PNG_THREADS) {
        const uint32_t v = png_filtered_at(s, p);
        f[png_ix8(p)] = (uint8_t)v;
        A += v;
        B += (uint32_t)(s.n - p) * v;                   // < 2^23 a term, 128 terms
    }
    l.red[tid] = A % PNG_ADLER;
    l.red2[tid] = B % PNG_ADLER;
}

// 1: per candidate, how many of the thread's bytes from its first on match their partner; every byte's position into its bucket
PNG_HD void png_step_lead(PngLds& l, const PngSeg& s, int tid)
{
    const uint8_t* f = reinterpret_cast<const uint8_t*>(l.b);
    const int c0 = tid * PNG_OWN, len = png_own(s, tid);
    for (int q = 0; q < PNG_CANDIDATES; q++) {
        const int d = png_distance(s, q);
        int k = 0;
        while (k < len && c0 + k >= d && f[png_ix8(c0 + k)] == f[png_ix8(c0 + k - d)]) k++;
        l.lead[q][tid] = (uint16_t)k;
    }
    for (int p = tid; p + PNG_HASH_MIN <= s.n; p += PNG_THREADS) {
        const uint32_t g = (uint32_t)f[png_ix8(p)] | ((uint32_t)f[png_ix8(p + 1)] << 8) | ((uint32_t)f[png_ix8(p + 2)] << 16) |
                           ((uint32_t)f[png_ix8(p + 3)] << 24);
        PNG_MIN(&l.htab[png_bucket(g)], (uint32_t)p);
    }
}

// 2: the best candidate of every byte of the thread, from its last byte backwards
PNG_HD void png_step_match(PngLds& l, const PngSeg& s, int tid)
{
    const uint8_t* f = reinterpret_cast<const uint8_t*>(l.b);
    const int c0 = tid * PNG_OWN, len = png_own(s, tid);
    int run[PNG_CANDIDATES], dist[PNG_CANDIDATES];
    for (int q = 0; q < PNG_CANDIDATES; q++) {
        dist[q] = png_distance(s, q);
        int acc = 0;                                     // the run that goes on behind the thread's last byte
        for (int t = tid + 1; t < PNG_THREADS; t++) {
            const int k = l.lead[q][t];
            acc += k;
            if (k < PNG_OWN || acc >= 258) break;
        }
        run[q] = len == PNG_OWN ? acc : 0;
    }
    uint32_t g = 0;                                      // the four bytes from j on, the first lowest
    for (int k = 2; k >= 0; k--) g = (g << 8) | (c0 + len + k < s.n ? (uint32_t)f[png_ix8(c0 + len + k)] : 0u);
    for (int j = c0 + len - 1; j >= c0; j--) {
        const uint32_t x = f[png_ix8(j)];
        g = (g << 8) | x;
        int best = 0, bq = 0;
        for (int q = 0; q < PNG_CANDIDATES; q++) {
            const int d = dist[q];
            run[q] = (j >= d && f[png_ix8(j - d)] == x) ? run[q] + 1 : 0;
            const int c = run[q] < 258 ? run[q] : 258;
            if (c > best) { best = c; bq = q; }
        }
        uint32_t mm = best >= 3 ? 0x8000u | ((uint32_t)bq << 8) | (uint32_t)(best - 3) : x;
        if (j + PNG_HASH_MIN <= s.n && best < PNG_HASH_MAX) {
            const uint32_t h = png_bucket(g), p = l.htab[h];
            if (p < (uint32_t)j) {
                int k = 0;
                while (k < PNG_HASH_MAX && j + k < s.n && f[png_ix8(j + k)] == f[png_ix8((int)p + k)]) k++;
                if (k >= PNG_HASH_MIN && k > best) mm = 0xc000u | ((uint32_t)(k - PNG_HASH_MIN) << 12) | h;
            }
        }
        l.m[png_ix16(j)] = (uint16_t)mm;
    }
}

// 3: the exit table over b (the filtered bytes are done with)
PNG_HD void png_step_exit(PngLds& l, const PngSeg& s, int tid)
{
    uint16_t* e = reinterpret_cast<uint16_t*>(l.b);
    const int c0 = tid * PNG_OWN, c1 = c0 + png_own(s, tid);
    for (int j = c1 - 1; j >= c0; j--) {
        const int nx = png_next(j, l.m[png_ix16(j)]);
        e[png_ix16(j)] = (uint16_t)(nx >= c1 ? nx : e[png_ix16(nx)]);
    }
}

// 4: thread 0 walks from thread to thread and notes where the parse enters each; the last thread adds up the Adler sums
// (red and red2 still hold step 0's)
PNG_HD void png_step_chain(PngLds& l, const PngSeg& s, int tid)
{
    if (tid == 0 && s.level >= 1) {
        const uint16_t* e = reinterpret_cast<const uint16_t*>(l.b);
        int pos = 0;
        while (pos < s.n) {
            l.entry[pos >> PNG_OWN_SHIFT] = (uint16_t)pos;
            pos = e[png_ix16(pos)];
        }
    }
    if (tid == PNG_THREADS - 1) {
        uint32_t a = 0, b = 0;
        for (int t = 0; t < PNG_THREADS; t++) {
            a += l.red[t];
            b += l.red2[t];
        }
        l.adler_a = a % PNG_ADLER;
        l.adler_b = b % PNG_ADLER;
    }
}

// 5: the bits of the thread's tokens
PNG_HD void png_step_count(PngLds& l, const PngSeg& s, int tid)
{
    const int c1 = tid * PNG_OWN + png_own(s, tid);
    uint32_t bits = 0;
    int j = l.entry[tid];
    if (j != (int)PNG_NONE) {
        while (j < c1) {
            const uint32_t mm = l.m[png_ix16(j)];
            int nb;
            png_token(l, s, mm, j, &nb);
            bits += (uint32_t)nb;
            j = png_next(j, mm);
        }
    }
    l.red[tid] = bits;
}

// 6: every thread's first bit, the total, and b cleared for the chunk
PNG_HD void png_step_scan(PngLds& l, const PngSeg& s, int tid)
{
    uint32_t before = 0, total = 0;
    for (int t = 0; t < PNG_THREADS; t++) {
        const uint32_t v = l.red[t];
        total += v;
        if (t < tid) before += v;
    }
    l.red2[tid] = before;
    if (tid == 0) l.total_bits = total;
    const int words = (GFT_PNG_CHUNK_SLOT + 3) / 4 + 2;
    for (int w = tid; w < words; w += PNG_THREADS) l.b[w] = 0;
    (void)s;
}

// 7: the chunk's bytes into b, all by OR into the cleared words: length, "IDAT", data
PNG_HD void png_step_emit(PngLds& l, const PngSeg& s, int tid)
{
    const PngForm f = png_form(s, l.total_bits);
    const int data0 = 8 + f.hdr;
    if (tid == 0) {
        for (int k = 0; k < 4; k++) png_or_byte(l.b, k, ((uint32_t)f.data_bytes >> (24 - 8 * k)) & 255u);
        png_or_byte(l.b, 4, 'I');
        png_or_byte(l.b, 5, 'D');
        png_or_byte(l.b, 6, 'A');
        png_or_byte(l.b, 7, 'T');
        if (f.hdr) {
            png_or_byte(l.b, 8, 0x78);
            png_or_byte(l.b, 9, 0x01);
        }
    }
    if (f.fixed) {
        if (tid == 0) {
            png_or_bits(l.b, (uint32_t)data0 * 8u, 2u);                        // BFINAL 0, BTYPE 01
            const int tail = data0 + (int)((f.bits + 7u) >> 3);                // 00 00 FF FF behind the padding
            png_or_byte(l.b, tail + 2, 0xff);
            png_or_byte(l.b, tail + 3, 0xff);
        }
        const int c1 = tid * PNG_OWN + png_own(s, tid);
        uint32_t at = (uint32_t)data0 * 8u + 3u + l.red2[tid];
        int j = l.entry[tid];
        if (j != (int)PNG_NONE) {
            while (j < c1) {
                const uint32_t mm = l.m[png_ix16(j)];
                int nb;
                const uint32_t bits = png_token(l, s, mm, j, &nb);
                png_or_bits(l.b, at, bits);
                at += (uint32_t)nb;
                j = png_next(j, mm);
            }
        }
    } else {
        if (tid == 0) {
            const uint32_t n = (uint32_t)s.n & 0xffffu, inv = ~(uint32_t)s.n & 0xffffu;      // n = 32768 fits
            png_or_byte(l.b, data0 + 1, n & 255u);
            png_or_byte(l.b, data0 + 2, n >> 8);
            png_or_byte(l.b, data0 + 3, inv & 255u);
            png_or_byte(l.b, data0 + 4, inv >> 8);
        }
        for (int p = tid; p < s.n; p += PNG_THREADS) png_or_byte(l.b, data0 + 5 + p, png_filtered_at(s, p));
    }
}

// 8: the CRC of the thread's piece of "IDAT" + data; the pieces are counted from the end, so all but the first are whole
PNG_HD void png_step_crc(PngLds& l, const PngSeg& s, int tid)
{
    const PngForm f = png_form(s, l.total_bits);
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(l.b);
    const int end = 8 + f.data_bytes;
    int hi = end - tid * PNG_PIECE, lo = hi - PNG_PIECE;
    if (lo < 4) lo = 4;
    uint32_t c = 0;
    if (hi > lo) {
        c = 0xffffffffu;
        for (int i = lo; i < hi; i++) c = l.crc_table[(c ^ bytes[i]) & 255u] ^ (c >> 8);
        c = ~c;
    }
    l.red[tid] = c;
}

// 9: sixteen threads fold sixteen pieces each, earliest bytes first
PNG_HD void png_step_fold(PngLds& l, const PngSeg& s, int tid)
{
    if (tid < PNG_THREADS / PNG_GROUP) {
        const int base = tid * PNG_GROUP;
        uint32_t c = l.red[base + PNG_GROUP - 1];
        for (int i = PNG_GROUP - 2; i >= 0; i--) c = png_mulmod(c, s.x2n_piece) ^ l.red[base + i];
        l.red2[tid] = c;
    }
}

// 10: thread 0 folds the sixteen and puts the CRC behind the data
PNG_HD void png_step_close(PngLds& l, const PngSeg& s, int tid)
{
    if (tid == 0) {
        const PngForm f = png_form(s, l.total_bits);
        const int groups = PNG_THREADS / PNG_GROUP;
        uint32_t c = l.red2[groups - 1];
        for (int i = groups - 2; i >= 0; i--) c = png_mulmod(c, s.x2n_group) ^ l.red2[i];
        for (int k = 0; k < 4; k++) png_or_byte(l.b, 8 + f.data_bytes + k, (c >> (24 - 8 * k)) & 255u);
    }
}

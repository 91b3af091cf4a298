// dn_inflate_core.hpp -- the one DEFLATE (RFC 1951) decoder of the library: the bit reader, the Huffman tables, the reading
// of a dynamic block's header, the symbol loop, the body over a span (inflate_span) and the two memory policies it runs
// against (HostMem, WaveMem).  dn_inflate.hip decodes BGZF blocks with it -- a block is the span from bit 0 with no history
// that stops at its final block and must give ISIZE bytes -- and dn_gz.hip the spans of a gzip stream.  __host__ __device__
// code; every unit that includes this header gets its own copy.
//
// A span starts at any bit, stops by a rule (Stop), reaches `have` bytes behind its entry and may not pass `limit` bytes.
// The policies carry a mode and the type of an output position (int32_t for a BGZF block, int64_t for a gzip segment):
//   kTrial    nothing is kept (rule 5 of a gzip guess)
//   kMarkers  the last 32 768 symbols as uint16 (a literal, or 0x8000 | j for byte j of the unknown 32 KiB before the entry);
//             finish() writes the ring in order: the tail
//   kBytes    bytes: the ring may be preloaded with history; WaveMem::flush() releases bytes [skip, skip + keep) to dst with
//             16-byte stores and runs the CRC over all of them, HostMem writes them in place
//
// Tables: a first-level lookup of 10 bits (literal/length) and 9 bits (distance) indexed by the next input bits, entry =
// symbol << 4 | code length, 0 = not in the table; longer codes (and codes that do not exist) take the canonical walk over
// count[len] / sorted symbols.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/degnorm_amd.h"
#include "dn_gz.hpp"

#ifndef DN_HD
#define DN_HD __host__ __device__ __forceinline__
#endif

#include "dn_crc.hpp"

namespace {

using dn::gz::Segment;

constexpr int kLitBits = 10, kDistBits = 9, kClBits = 7;
constexpr int kRing = 32768;                 // bytes of history in LDS (device)
constexpr int kWin = 2048;                   // bytes of payload in LDS (device)
constexpr int kHeaderBytes = 640;            // a dynamic block header is at most 3 + 14 + 57 + 316 * 14 bits = 563 bytes
constexpr int kSymbolBytes = 16;             // a length/distance pair is at most 48 bits; two refills of 4 bytes

struct Tables {
    uint16_t *lit, *dist;                    // first-level tables, 1 << kLitBits and 1 << kDistBits entries
    uint16_t *sym_l, *sym_d;                 // symbols sorted by code length, then by value (288 and 32)
    uint16_t *cnt_l, *cnt_d;                 // number of codes of each length (16 each)
    uint16_t *offs;                          // scratch of build_table (16)
    uint8_t *lens;                           // code lengths being read (320)
};

struct BitReader {
    uint64_t bb = 0;                         // bits not yet consumed, the next one lowest
    int32_t bc = 0;                          // how many of them
    int32_t next = 0;                        // payload offset of the next word to load
    int32_t n_in = 0;                        // payload bytes
};

template <class M> DN_HD void seek(BitReader &r, M &m, int32_t p)      // continue at payload byte p
{
    m.ensure_in(p, kHeaderBytes, r.n_in);
    const int32_t a = m.misalign(p);
    const uint32_t w = m.word(p - a, r.n_in);
    r.bb = (uint64_t) (w >> (8 * a));
    r.bc = 32 - 8 * a;
    r.next = p - a + 4;
}
template <class M> DN_HD void refill(BitReader &r, M &m)               // at least 33 bits afterwards
{
    if (r.bc <= 32) {
        r.bb |= (uint64_t) m.word(r.next, r.n_in) << r.bc;
        r.bc += 32;
        r.next += 4;
    }
}
DN_HD uint32_t peek(const BitReader &r, int n) { return (uint32_t) r.bb & ((1u << n) - 1u); }
DN_HD void drop(BitReader &r, int n) { r.bb >>= n; r.bc -= n; }
DN_HD uint32_t take(BitReader &r, int n) { const uint32_t v = peek(r, n); drop(r, n); return v; }
DN_HD int64_t bits_used(const BitReader &r) { return (int64_t) r.next * 8 - r.bc; }
DN_HD bool overrun(const BitReader &r) { return bits_used(r) > (int64_t) r.n_in * 8; }

DN_HD uint32_t reverse_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// Canonical Huffman code of lens[0 .. n): cnt, sym and the first-level table of `bits` bits.  0, or DN_INFLATE_E_LENGTHS for
// an over-subscribed set or an incomplete one (zlib's rule: a lone code of one bit may stay incomplete when `lone_ok`).
template <class M>
DN_HD int build_table(M &m, const uint8_t *lens, int n, uint16_t *cnt, uint16_t *sym, uint16_t *offs, uint16_t *tab, int bits, bool lone_ok)
{
    for (int l = 0; l < 16; l++) m.set(cnt + l, 0);
    for (int i = 0; i < n; i++) { const int l = lens[i] & 15; m.set(cnt + l, (uint16_t) (cnt[l] + 1)); }
    for (int k = 0; k < (1 << bits); k += M::kLanes) m.set_lane(tab + k, 0);
    if (cnt[0] == n) return 0;                                  // no codes: every lookup fails
    int left = 1, max = 0;
    for (int l = 1; l < 16; l++) {
        left = (left << 1) - (int) cnt[l];
        if (left < 0) return DN_INFLATE_E_LENGTHS;
        if (cnt[l]) max = l;
    }
    if (left > 0 && !(lone_ok && max == 1)) return DN_INFLATE_E_LENGTHS;
    m.set(offs + 1, 0);
    for (int l = 1; l < 15; l++) m.set(offs + l + 1, (uint16_t) (offs[l] + cnt[l]));
    for (int i = 0; i < n; i++) {
        const int l = lens[i] & 15;
        if (l) { const int o = offs[l]; m.set(sym + o, (uint16_t) i); m.set(offs + l, (uint16_t) (o + 1)); }
    }
    uint32_t code = 0;
    int index = 0;
    for (int l = 1; l <= bits && l <= max; l++) {
        const int c = cnt[l];
        for (int j = 0; j < c; j++) {
            const uint16_t e = (uint16_t) ((sym[index + j] << 4) | l);
            for (uint32_t k = reverse_bits(code + j, l); k < (1u << bits); k += 1u << l) m.set(tab + k, e);
        }
        index += c;
        code = (code + c) << 1;
    }
    return 0;
}

// the symbol of the next code: first-level table, else the canonical walk; -1 when no code matches.  Needs 15 bits.
DN_HD int decode_symbol(BitReader &r, const uint16_t *tab, int bits, const uint16_t *cnt, const uint16_t *sym)
{
    const uint32_t e = tab[peek(r, bits)];
    if (e) { drop(r, e & 15); return (int) (e >> 4); }
    int code = 0, first = 0, index = 0;
    uint32_t b = (uint32_t) r.bb;
    for (int l = 1; l < 16; l++) {
        code |= (int) (b & 1u);
        b >>= 1;
        const int c = cnt[l];
        if (code - c < first) { drop(r, l); return sym[index + (code - first)]; }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

template <class M> DN_HD int read_dynamic(BitReader &r, M &m, const Tables &t, int &n_lit, int &n_dist)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    refill(r, m);
    n_lit = (int) take(r, 5) + 257;
    n_dist = (int) take(r, 5) + 1;
    const int n_cl = (int) take(r, 4) + 4;
    if (n_lit > 286 || n_dist > 30) return DN_INFLATE_E_HEADER;
    for (int i = 0; i < 19; i++) m.set8(t.lens + i, 0);
    for (int i = 0; i < n_cl; i++) { refill(r, m); m.set8(t.lens + order[i], (uint8_t) take(r, 3)); }
    int rc = build_table(m, t.lens, 19, t.cnt_l, t.sym_l, t.offs, t.lit, kClBits, false);
    if (rc) return rc;
    int i = 0, prev = 0;
    while (i < n_lit + n_dist) {
        refill(r, m);
        const uint32_t e = t.lit[peek(r, kClBits)];
        if (!e) return DN_INFLATE_E_LENGTHS;
        drop(r, e & 15);
        const int s = (int) (e >> 4);
        if (s < 16) { m.set8(t.lens + i++, (uint8_t) s); prev = s; continue; }
        int rep, v = 0;
        if (s == 16) { if (i == 0) return DN_INFLATE_E_LENGTHS; v = prev; rep = 3 + (int) take(r, 2); }
        else if (s == 17) rep = 3 + (int) take(r, 3);
        else rep = 11 + (int) take(r, 7);
        if (i + rep > n_lit + n_dist) return DN_INFLATE_E_LENGTHS;
        for (int k = 0; k < rep; k++) m.set8(t.lens + i++, (uint8_t) v);
        prev = v;
    }
    if (overrun(r)) return DN_INFLATE_E_INPUT;
    if (t.lens[256] == 0) return DN_INFLATE_E_LENGTHS;          // no end-of-block code
    return 0;
}

constexpr int kHist = dn::gz::kHistory;
constexpr int kTrial = 0, kMarkers = 1, kBytes = 2;
constexpr int64_t kNoLimit = INT64_MAX;

// where a span's decode ends, tested at the end of every block that is not final
struct Stop {
    enum { kBlock, kReach, kGuess, kFinal };   // kFinal: only a final block ends the span
    int32_t mode, shift;                     // shift: log2 of the bits of a chunk
    int64_t bit;                             // kReach: the first block end at or beyond this bit
    const int64_t *guess;                    // kGuess: the first block end that is the guess of its chunk
    int64_t n_chunks;
    bool whole = false;                      // the input is all there is (a BGZF payload): bits beyond it are an error, not a cut
    DN_HD bool hit(int64_t y) const
    {
        if (mode == kBlock) return true;
        if (mode == kFinal) return false;
        if (mode == kReach) return y >= bit;
        const int64_t k = y >> shift;
        return k < n_chunks && guess[k] == y;
    }
};

// no code matched the next 15 bits, and some of them lie beyond the span: the span is cut, the code is not known to be bad
DN_HD bool peeked_beyond(const BitReader &r) { return bits_used(r) + 15 > (int64_t) r.n_in * 8; }

// the symbols of a block whose tables are built, up to its end-of-block code.  0 or DN_INFLATE_E_*.
template <class M>
DN_HD int symbols(BitReader &r, M &m, const Tables &t, int32_t n_in, typename M::Pos &out_pos, typename M::Pos have, typename M::Pos limit, bool whole)
{
    for (;;) {
        m.ensure_in(r.next, kSymbolBytes, n_in);
        m.ensure_out(out_pos, 258);
        refill(r, m);
        int s = decode_symbol(r, t.lit, kLitBits, t.cnt_l, t.sym_l);
        if (s < 0) return (whole ? overrun(r) : peeked_beyond(r)) ? DN_INFLATE_E_INPUT : DN_INFLATE_E_CODE;
        if (s < 256) {
            if (overrun(r)) return DN_INFLATE_E_INPUT;
            if (out_pos >= limit) return DN_INFLATE_E_SIZE;
            m.put(out_pos++, (uint8_t) s);
            continue;
        }
        if (s == 256) return overrun(r) ? DN_INFLATE_E_INPUT : 0;
        s -= 257;
        if (s >= 29) return DN_INFLATE_E_CODE;
        int len;
        if (s < 8) len = 3 + s;
        else if (s == 28) len = 258;
        else { const int e = (s - 4) >> 2; len = 3 + ((4 + (s & 3)) << e) + (int) take(r, e); }
        refill(r, m);
        int d = decode_symbol(r, t.dist, kDistBits, t.cnt_d, t.sym_d);
        if (d < 0) return (whole ? overrun(r) : peeked_beyond(r)) ? DN_INFLATE_E_INPUT : DN_INFLATE_E_CODE;
        if (d >= 30) return DN_INFLATE_E_CODE;
        int dist;
        if (d < 4) dist = 1 + d;
        else { const int e = (d - 2) >> 1; dist = 1 + ((2 + (d & 1)) << e) + (int) take(r, e); }
        if (overrun(r)) return DN_INFLATE_E_INPUT;
        if (dist > out_pos + have) return DN_INFLATE_E_DISTANCE;
        if (len > limit - out_pos) return DN_INFLATE_E_SIZE;
        m.copy(out_pos, dist, len);
        out_pos += len;
    }
}

template <class M> DN_HD void seek_bit(BitReader &r, M &m, int64_t bit)
{
    seek(r, m, (int32_t) (bit >> 3));
    drop(r, (int) (bit & 7));
}

DN_HD bool complete(const uint16_t *cnt)
{
    int left = 1;
    for (int l = 1; l < 16; l++) left = (left << 1) - (int) cnt[l];
    return left == 0;
}

// The blocks of a span of n_in bytes from bit `entry` to where `stop` says, or to the end of a final block.  The history
// reaches `have` bytes behind the entry, the output may not pass `limit` bytes.  o.status = 0 or DN_INFLATE_E_*; every trip
// of the block loop and of the symbol loop consumes at least one bit and ends on the first bit beyond the span.
template <class M>
DN_HD void inflate_span(M &m, const Tables &t, int32_t n_in, int64_t entry, const Stop &stop, typename M::Pos have, typename M::Pos limit, Segment &o)
{
    BitReader r;
    r.n_in = n_in;
    typename M::Pos out_pos = 0;
    o.entry = entry; o.exit = entry; o.out_len = 0; o.kind = DN_GZ_EXIT_BLOCK; o.blocks = 0; o.pad = 0;
    seek_bit(r, m, entry);
    for (;;) {
        m.ensure_in(r.next, kHeaderBytes, n_in);
        refill(r, m);
        const bool last = take(r, 1) != 0;
        const uint32_t type = take(r, 2);
        int rc = 0;
        if (overrun(r)) rc = DN_INFLATE_E_INPUT;
        else if (type == 3) rc = DN_INFLATE_E_HEADER;
        else if (type == 0) {
            const int64_t p = (bits_used(r) + 7) >> 3;          // LEN and NLEN start at the next byte boundary
            if (p + 4 > n_in) rc = DN_INFLATE_E_INPUT;
            else {
                seek(r, m, (int32_t) p);
                refill(r, m);
                const uint32_t len = take(r, 16), nlen = take(r, 16);
                if ((len ^ nlen) != 0xffffu) rc = DN_INFLATE_E_HEADER;
                else if (p + 4 + len > n_in) rc = DN_INFLATE_E_INPUT;
                else if ((int64_t) len > limit - out_pos) rc = DN_INFLATE_E_SIZE;
                else {
                    m.stored((int32_t) p + 4, (int32_t) len, out_pos);
                    out_pos += (typename M::Pos) len;
                    seek(r, m, (int32_t) p + 4 + (int32_t) len);
                }
            }
        } else {
            int n_lit = 288, n_dist = 32;
            if (type == 1) {
                for (int i = 0; i < 288; i++) m.set8(t.lens + i, (uint8_t) (i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8));
                for (int i = 288; i < 320; i++) m.set8(t.lens + i, 5);
            } else {
                rc = read_dynamic(r, m, t, n_lit, n_dist);
            }
            if (rc == 0) rc = build_table(m, t.lens, n_lit, t.cnt_l, t.sym_l, t.offs, t.lit, kLitBits, true);
            if (rc == 0) rc = build_table(m, t.lens + n_lit, n_dist, t.cnt_d, t.sym_d, t.offs, t.dist, kDistBits, true);
            if (rc == 0) rc = symbols(r, m, t, n_in, out_pos, have, limit, stop.whole);
        }
        if (rc) {                                               // found on bits beyond a span that may be cut: a cut, nothing else is known
            o.status = !stop.whole && overrun(r) ? DN_INFLATE_E_INPUT : rc;
            return;
        }
        o.blocks++;
        const int64_t y = bits_used(r);
        if (last || stop.hit(y)) {
            o.exit = y; o.out_len = out_pos; o.kind = last ? DN_GZ_EXIT_MEMBER : DN_GZ_EXIT_BLOCK; o.status = 0;
            m.finish(out_pos);
            return;
        }
    }
}

// the CRC register c after n bytes too: what the lanes' slices of WaveMem::flush join to, a byte at a time
uint32_t crc_bytes(uint32_t c, const uint8_t *data, int64_t n)
{
    struct Table {
        uint32_t v[256];
        Table() { for (uint32_t b = 0; b < 256; b++) v[b] = crc_bits(b, 8); }
    };
    static const Table table;
    for (int64_t i = 0; i < n; i++) c = table.v[(c ^ data[i]) & 0xffu] ^ (c >> 8);
    return c;
}

// --- host: plain arrays ---------------------------------------------------------------------------------------------------

template <int kMode, class PosT> struct HostMem {
    static constexpr int kLanes = 1;
    using Pos = PosT;
    using Sym = typename std::conditional<kMode == kMarkers, uint16_t, uint8_t>::type;
    const uint8_t *in;              // the span
    Sym *ring;                      // kHist symbols (kTrial: none)
    uint8_t *out;                   // kBytes: the segment's place
    uint16_t *tail;                 // kMarkers: kHist symbols
    bool check;                     // keep the CRC register
    uint32_t crc = 0;               // where the register starts

    void ensure_in(int32_t, int32_t, int32_t) {}
    void ensure_out(Pos, int32_t) {}
    int32_t misalign(int32_t) const { return 0; }
    uint32_t word(int32_t p, int32_t n_in) const
    {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++)
            if (p + k >= 0 && p + k < n_in) w |= (uint32_t) in[p + k] << (8 * k);
        return w;
    }
    void set(uint16_t *p, uint16_t v) { *p = v; }
    void set_lane(uint16_t *p, uint16_t v) { *p = v; }
    void set8(uint8_t *p, uint8_t v) { *p = v; }
    void put(Pos pos, uint8_t v)
    {
        if (kMode != kTrial) ring[pos & (kHist - 1)] = v;
        if (kMode == kBytes) out[pos] = v;
    }
    void copy(Pos pos, int32_t dist, int32_t len)
    {
        if (kMode == kTrial) return;
        for (int32_t i = 0; i < len; i++) {
            const Sym v = ring[(pos + i - dist) & (kHist - 1)];
            ring[(pos + i) & (kHist - 1)] = v;
            if (kMode == kBytes) out[pos + i] = (uint8_t) v;
        }
    }
    void stored(int32_t src, int32_t len, Pos pos)
    {
        for (int32_t i = 0; i < len; i++) put(pos + i, in[src + i]);
    }
    void finish(Pos pos)
    {
        if (kMode == kMarkers)
            for (int j = 0; j < kHist; j++) tail[j] = (uint16_t) ring[(pos + j) & (kHist - 1)];
        if (kMode == kBytes && check) crc = crc_bytes(crc, out, pos);
    }
};

// --- device: one wave -------------------------------------------------------------------------------------------------------

struct RingReader {
    const uint32_t *ring32;
    __device__ __forceinline__ uint32_t dword(int32_t p) const { return ring32[(uint32_t) (p >> 2) & (kRing / 4 - 1)]; }
};

// the CRC register reg after the ring's bytes [a, b) too (a call: the symbol loop stays small)
__device__ __noinline__ uint32_t wave_crc(const uint8_t *ring, uint32_t reg, int32_t a, int32_t b, int32_t lane)
{
    uint32_t x = crc_slice(RingReader{reinterpret_cast<const uint32_t *>(ring)}, a, b, lane, 64);
    for (int o = 32; o > 0; o >>= 1) x ^= (uint32_t) __shfl_xor((int) x, o, 64);
    return crc_join(reg, x, a, b);
}

template <int kMode, class PosT> struct WaveMem {
    static constexpr int kLanes = 64;
    using Pos = PosT;
    using Sym = typename std::conditional<kMode == kMarkers, uint16_t, uint8_t>::type;
    Sym *ring;                      // LDS, kHist symbols (kTrial: none)
    uint32_t *win;                  // LDS, kWin bytes: comp[wbase .. wbase + kWin)
    const uint8_t *comp;            // 16-byte aligned, comp_cap bytes in whole 16-byte pieces
    int64_t comp_cap, abs0, wbase;  // abs0: the input's offset in comp; wbase: a multiple of 16
    int32_t lane;
    uint8_t *dst;                   // kBytes: where byte `skip` of the output goes
    uint16_t *tail;                 // kMarkers: kHist symbols, 16-byte aligned
    Pos skip, keep, flushed;        // kBytes: bytes [skip, skip + keep) of the output are kept
    bool check;
    uint32_t crc;

    __device__ __forceinline__ void fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

    __device__ __forceinline__ void ensure_in(int32_t p, int32_t k, int32_t n_in)
    {
        const int64_t a = abs0 + p;
        int64_t need = a + k;
        if (need > abs0 + n_in) need = abs0 + n_in;
        if (a >= wbase && need <= wbase + kWin) return;
        wbase = a & ~(int64_t) 15;
        fence();
        for (int j = lane; j < kWin / 16; j += 64) {
            const int64_t o = wbase + 16 * (int64_t) j;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (o >= 0 && o + 16 <= comp_cap) v = *reinterpret_cast<const uint4 *>(comp + o);
            reinterpret_cast<uint4 *>(win)[j] = v;
        }
        fence();
    }
    __device__ __forceinline__ int32_t misalign(int32_t p) const { return (int32_t) ((abs0 + p) & 3); }
    __device__ __forceinline__ uint32_t word(int32_t p, int32_t n_in) const      // bytes beyond the span read as 0, as on the host
    {
        const uint32_t w = win[(uint32_t) ((abs0 + p - wbase) >> 2) & (kWin / 4 - 1)];
        if (p + 4 <= n_in) return w;
        return p >= n_in ? 0u : w & (0xffffffffu >> (8 * (p + 4 - n_in)));
    }
    __device__ __forceinline__ void set(uint16_t *p, uint16_t v) { if (lane == 0) *p = v; fence(); }
    __device__ __forceinline__ void set_lane(uint16_t *p, uint16_t v) { p[lane] = v; fence(); }
    __device__ __forceinline__ void set8(uint8_t *p, uint8_t v) { if (lane == 0) *p = v; fence(); }
    __device__ __forceinline__ void put(Pos pos, uint8_t v)
    {
        if (kMode == kTrial) return;
        if (lane == 0) ring[(uint32_t) pos & (kHist - 1)] = v;
        fence();
    }

    // out[pos .. pos + len) = out[pos - dist ..): every lane a symbol; a period shorter than the wave doubles each step
    __device__ __forceinline__ void copy(Pos pos, int32_t dist, int32_t len)
    {
        if (kMode == kTrial) return;
        const uint32_t p0 = (uint32_t) pos;
        int32_t done = 0, d = dist;
        while (done < len) {
            int32_t step = d < 64 ? d : 64;
            if (step > len - done) step = len - done;
            Sym v = 0;
            if (lane < step) v = ring[(p0 + done + lane - d) & (kHist - 1)];
            fence();
            if (lane < step) ring[(p0 + done + lane) & (kHist - 1)] = v;
            fence();
            done += step;
            if (d < 64) d += d;
        }
    }

    // kBytes: ring bytes [flushed, to) -> dst, the part inside [skip, skip + keep); all of them into the CRC register
    __device__ __forceinline__ void flush(Pos to)
    {
        fence();
        if (to <= flushed) return;
        const uint8_t *ring8 = reinterpret_cast<const uint8_t *>(ring);
        if (check) {
            const int32_t a = (int32_t) (flushed & (kHist - 1));
            crc = wave_crc(ring8, crc, a, a + (int32_t) (to - flushed), lane);
        }
        const Pos lo = flushed > skip ? flushed : skip, hi = to < skip + keep ? to : skip + keep;
        flushed = to;
        if (lo >= hi) return;
        uint8_t *d0 = dst - skip;                               // where byte 0 of the output would go
        Pos head = (Pos) ((0 - (reinterpret_cast<uintptr_t>(d0) + (uintptr_t) lo)) & 15u);
        if (head > hi - lo) head = hi - lo;
        if (lane < head) d0[lo + lane] = ring8[(uint32_t) (lo + lane) & (kHist - 1)];
        const Pos body = lo + head;
        const int32_t n_vec = (int32_t) ((hi - body) >> 4);
        const uint32_t *ring32 = reinterpret_cast<const uint32_t *>(ring);
        for (int32_t v = lane; v < n_vec; v += 64) {
            const Pos s = body + 16 * (Pos) v;
            const uint32_t sh = 8u * (uint32_t) (s & 3), i0 = (uint32_t) (s >> 2);
            uint32_t w[5];
            for (int k = 0; k < 5; k++) w[k] = ring32[(i0 + k) & (kHist / 4 - 1)];
            uint4 q;
            q.x = (uint32_t) ((((uint64_t) w[1] << 32) | w[0]) >> sh);
            q.y = (uint32_t) ((((uint64_t) w[2] << 32) | w[1]) >> sh);
            q.z = (uint32_t) ((((uint64_t) w[3] << 32) | w[2]) >> sh);
            q.w = (uint32_t) ((((uint64_t) w[4] << 32) | w[3]) >> sh);
            *reinterpret_cast<uint4 *>(d0 + s) = q;
        }
        const Pos rest = body + 16 * (Pos) n_vec;
        if (rest + lane < hi) d0[rest + lane] = ring8[(uint32_t) (rest + lane) & (kHist - 1)];
    }
    __device__ __forceinline__ void ensure_out(Pos pos, int32_t k)
    {
        if (kMode == kBytes && pos + k - flushed > kHist) flush(pos);
    }
    __device__ __forceinline__ void stored(int32_t src, int32_t len, Pos pos)
    {
        if (kMode == kTrial) return;
        while (len > 0) {
            int32_t chunk = len;
            if (kMode == kBytes) {
                if (pos - flushed >= kHist) flush(pos);
                if (chunk > kHist - (int32_t) (pos - flushed)) chunk = kHist - (int32_t) (pos - flushed);
            }
            const uint32_t p0 = (uint32_t) pos;
            for (int32_t i = lane; i < chunk; i += 64) ring[(p0 + i) & (kHist - 1)] = comp[abs0 + src + i];
            fence();
            src += chunk; pos += chunk; len -= chunk;
        }
    }
    __device__ __forceinline__ void finish(Pos pos)
    {
        if (kMode == kBytes) flush(pos);
        if (kMode == kMarkers) {
            fence();
            const uint32_t p0 = (uint32_t) pos;
            for (int v = lane; v < kHist / 8; v += 64) {
                uint32_t w[4];
                for (int k = 0; k < 4; k++) {
                    const uint32_t a = ring[(p0 + 8 * v + 2 * k) & (kHist - 1)], b = ring[(p0 + 8 * v + 2 * k + 1) & (kHist - 1)];
                    w[k] = a | (b << 16);
                }
                reinterpret_cast<uint4 *>(tail)[v] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    }
};

}  // namespace

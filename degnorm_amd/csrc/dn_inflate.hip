// dn_inflate.hip -- raw DEFLATE (RFC 1951) decoder for BGZF blocks, one block per wavefront.
//
// A BGZF block is an independent raw-deflate stream of at most 64 KiB that names its own inflated size (ISIZE), so the
// blocks of a window inflate side by side.  The decoder below (inflate_block) is written once, as __host__ __device__ code
// against a memory policy M that says how input words, output bytes and the window of history are reached:
//
//   HostMem   plain arrays: the payload is read with bounds-checked loads, the output is written in place.  This is what
//             dn_bgzf_inflate_host runs, block after block, without a device: the build that is debugged and fuzzed.
//   WaveMem   one 64-lane workgroup (one wave) per block.  All 64 lanes run the bit reader and the symbol loop on the same
//             state (SIMT executes them at the price of one), so every branch is wave-uniform and nothing has to be
//             handed from a "decoding lane" to the others: a literal is stored by lane 0, a match is copied by all lanes,
//             and window refills and flushes are ordinary calls.  In LDS: the last 32 KiB of output as a ring (DEFLATE
//             reaches back at most 32768 bytes), a 2 KiB window of the payload, and the Huffman tables (38.9 KiB in
//             all: four workgroups per CU).  LDS operations of one wave execute in order, so a back-reference reads
//             what earlier instructions of the wave stored; wavefront-scope fences keep the compiler from reordering
//             them.  The ring is flushed to global memory with 16-byte stores before unflushed bytes would be
//             overwritten, and at the end.
//
// CRC32: with InflateBlock::check the policy keeps a running CRC register over every inflated byte (crc_slice, crc_join below).
// WaveMem does it in flush(), on the bytes the ring is about to release: every lane takes one contiguous slice from register
// 0, shifts it by the bytes behind it, and an xor across the wave joins the slices to the register carried from the flush
// before.  Bit by bit, without a table: no LDS beyond the 38.9 KiB above; measured, the pass adds 1.7-1.9 % to the kernel
// (about 5 cycles per byte against the 250 of the symbol loop; DESIGN.md, "BGZF inflate").  HostMem runs the same routines
// over its output array, lane after lane.
//
// Tables: a first-level lookup of 10 bits (literal/length) and 9 bits (distance) indexed by the next input bits, entry =
// symbol << 4 | code length, 0 = not in the table; longer codes (and codes that do not exist) take the canonical walk over
// count[len] / sorted symbols.  Input is untrusted: DESIGN.md ("BGZF inflate") has the bounds argument.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_inflate.hpp"

#define DN_HD __host__ __device__ __forceinline__
#include "dn_crc.hpp"

namespace {

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

// Inflate one payload of n_in bytes into exactly isize bytes.  0 or DN_INFLATE_E_*.  Every trip of the block loop and of the
// symbol loop consumes at least one bit and ends on the first bit beyond the payload, so both are bounded by 8 * n_in.
// With m.check the block must also have the CRC32 `crc`; a decode error wins over DN_INFLATE_E_CRC.
template <class M> DN_HD int inflate_block(M &m, const Tables &t, int32_t n_in, int32_t isize, uint32_t crc)
{
    BitReader r;
    r.n_in = n_in;
    int32_t out_pos = 0;
    seek(r, m, 0);
    for (bool last = false; !last;) {
        m.ensure_in(r.next, kHeaderBytes, n_in);
        refill(r, m);
        last = take(r, 1) != 0;
        const uint32_t type = take(r, 2);
        if (overrun(r)) return DN_INFLATE_E_INPUT;
        if (type == 3) return DN_INFLATE_E_HEADER;
        if (type == 0) {
            const int64_t p = (bits_used(r) + 7) >> 3;          // LEN and NLEN start at the next byte boundary
            if (p + 4 > n_in) return DN_INFLATE_E_INPUT;
            seek(r, m, (int32_t) p);
            refill(r, m);
            const uint32_t len = take(r, 16), nlen = take(r, 16);
            if ((len ^ nlen) != 0xffffu) return DN_INFLATE_E_HEADER;
            if (p + 4 + len > n_in) return DN_INFLATE_E_INPUT;
            if ((int64_t) out_pos + len > isize) return DN_INFLATE_E_SIZE;
            m.stored((int32_t) p + 4, (int32_t) len, out_pos);
            out_pos += (int32_t) len;
            seek(r, m, (int32_t) p + 4 + (int32_t) len);
            continue;
        }
        int n_lit = 288, n_dist = 32;
        if (type == 1) {
            for (int i = 0; i < 288; i++) m.set8(t.lens + i, (uint8_t) (i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8));
            for (int i = 288; i < 320; i++) m.set8(t.lens + i, 5);
        } else {
            const int rc = read_dynamic(r, m, t, n_lit, n_dist);
            if (rc) return rc;
        }
        int rc = build_table(m, t.lens, n_lit, t.cnt_l, t.sym_l, t.offs, t.lit, kLitBits, true);
        if (rc == 0) rc = build_table(m, t.lens + n_lit, n_dist, t.cnt_d, t.sym_d, t.offs, t.dist, kDistBits, true);
        if (rc) return rc;
        for (;;) {
            m.ensure_in(r.next, kSymbolBytes, n_in);
            m.ensure_out(out_pos, 258);
            refill(r, m);
            int s = decode_symbol(r, t.lit, kLitBits, t.cnt_l, t.sym_l);
            if (s < 0) return overrun(r) ? DN_INFLATE_E_INPUT : DN_INFLATE_E_CODE;
            if (s < 256) {
                if (overrun(r)) return DN_INFLATE_E_INPUT;
                if (out_pos >= isize) return DN_INFLATE_E_SIZE;
                m.put(out_pos++, (uint8_t) s);
                continue;
            }
            if (s == 256) {
                if (overrun(r)) return DN_INFLATE_E_INPUT;
                break;
            }
            s -= 257;
            if (s >= 29) return DN_INFLATE_E_CODE;
            int len;
            if (s < 8) len = 3 + s;
            else if (s == 28) len = 258;
            else { const int e = (s - 4) >> 2; len = 3 + ((4 + (s & 3)) << e) + (int) take(r, e); }
            refill(r, m);
            int d = decode_symbol(r, t.dist, kDistBits, t.cnt_d, t.sym_d);
            if (d < 0) return overrun(r) ? DN_INFLATE_E_INPUT : DN_INFLATE_E_CODE;
            if (d >= 30) return DN_INFLATE_E_CODE;
            int dist;
            if (d < 4) dist = 1 + d;
            else { const int e = (d - 2) >> 1; dist = 1 + ((2 + (d & 1)) << e) + (int) take(r, e); }
            if (overrun(r)) return DN_INFLATE_E_INPUT;
            if (dist > out_pos) return DN_INFLATE_E_DISTANCE;
            if (out_pos + len > isize) return DN_INFLATE_E_SIZE;
            m.copy(out_pos, dist, len);
            out_pos += len;
        }
    }
    if (out_pos != isize) return DN_INFLATE_E_SIZE;
    if (((bits_used(r) + 7) >> 3) != n_in) return DN_INFLATE_E_TRAILING;
    m.finish(out_pos);
    if (m.check && (m.crc ^ 0xffffffffu) != crc) return DN_INFLATE_E_CRC;
    return 0;
}

// --- host: plain arrays ---------------------------------------------------------------------------------------------------

struct HostMem {
    static constexpr int kLanes = 1;
    const uint8_t *in;              // the payload
    uint8_t *out;                   // isize bytes
    bool check;                     // keep the CRC register
    uint32_t crc = 0xffffffffu;

    void ensure_in(int32_t, int32_t, int32_t) {}
    void ensure_out(int32_t, int32_t) {}
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
    void put(int32_t pos, uint8_t v) { out[pos] = v; }
    void copy(int32_t pos, int32_t dist, int32_t len)
    {
        for (int32_t i = 0; i < len; i++) out[pos + i] = out[pos + i - dist];
    }
    void stored(int32_t src, int32_t len, int32_t pos) { memcpy(out + pos, in + src, (size_t) len); }
    void finish(int32_t pos) { if (check) crc = crc_host(crc, out, pos, 64, kRing); }      // sliced and cut as the device does
};

// --- device: one wave, history and payload window in LDS -----------------------------------------------------------------

struct RingReader {
    const uint32_t *ring32;
    __device__ __forceinline__ uint32_t dword(int32_t p) const { return ring32[(uint32_t) (p >> 2) & (kRing / 4 - 1)]; }
};

// the CRC register reg after the ring's bytes [a, b) too.  A call, not inline: flush() is inlined into the symbol loop, and
// the loop of a launch that checks nothing should stay the code it was.
__device__ __noinline__ uint32_t wave_crc(const uint8_t *ring, uint32_t reg, int32_t a, int32_t b, int32_t lane)
{
    uint32_t x = crc_slice(RingReader{reinterpret_cast<const uint32_t *>(ring)}, a, b, lane, 64);
    for (int o = 32; o > 0; o >>= 1) x ^= (uint32_t) __shfl_xor((int) x, o, 64);
    return crc_join(reg, x, a, b);
}

struct WaveMem {
    static constexpr int kLanes = 64;
    uint8_t *ring;                  // LDS, kRing bytes
    uint32_t *win;                  // LDS, kWin bytes: comp[wbase .. wbase + kWin)
    const uint8_t *comp;
    int64_t comp_cap, abs0, wbase;  // abs0: the payload's offset in comp; wbase: a multiple of 16
    uint8_t *dst;                   // where byte `skip` of the output goes
    int32_t skip, keep, flushed, lane;
    bool check;                     // keep the CRC register
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
    __device__ __forceinline__ uint32_t word(int32_t p, int32_t n_in) const      // bytes beyond the payload read as 0, as on the host
    {
        const uint32_t w = win[(uint32_t) ((abs0 + p - wbase) >> 2) & (kWin / 4 - 1)];
        if (p + 4 <= n_in) return w;
        return p >= n_in ? 0u : w & (0xffffffffu >> (8 * (p + 4 - n_in)));
    }
    __device__ __forceinline__ void set(uint16_t *p, uint16_t v) { if (lane == 0) *p = v; fence(); }
    __device__ __forceinline__ void set_lane(uint16_t *p, uint16_t v) { p[lane] = v; fence(); }
    __device__ __forceinline__ void set8(uint8_t *p, uint8_t v) { if (lane == 0) *p = v; fence(); }
    __device__ __forceinline__ void put(int32_t pos, uint8_t v) { if (lane == 0) ring[pos & (kRing - 1)] = v; fence(); }

    // out[pos .. pos + len) = out[pos - dist ..): every lane a byte; a period shorter than the wave doubles each step
    __device__ __forceinline__ void copy(int32_t pos, int32_t dist, int32_t len)
    {
        int32_t done = 0, d = dist;
        while (done < len) {
            int32_t step = d < 64 ? d : 64;
            if (step > len - done) step = len - done;
            uint8_t v = 0;
            if (lane < step) v = ring[(pos + done + lane - d) & (kRing - 1)];
            fence();
            if (lane < step) ring[(pos + done + lane) & (kRing - 1)] = v;
            fence();
            done += step;
            if (d < 64) d += d;
        }
    }

    // ring bytes [flushed, to) -> global memory, the part inside [skip, skip + keep); all of them into the CRC register
    __device__ __forceinline__ void flush(int32_t to)
    {
        fence();
        if (check && to > flushed) crc = wave_crc(ring, crc, flushed, to, lane);
        int32_t lo = flushed > skip ? flushed : skip, hi = to < skip + keep ? to : skip + keep;
        flushed = to;
        if (lo >= hi) return;
        int32_t head = (int32_t) ((0 - (reinterpret_cast<uintptr_t>(dst) + (uintptr_t) (lo - skip))) & 15u);
        if (head > hi - lo) head = hi - lo;
        if (lane < head) dst[lo - skip + lane] = ring[(lo + lane) & (kRing - 1)];
        const int32_t body = lo + head, n_vec = (hi - body) >> 4;
        const uint32_t *ring32 = reinterpret_cast<const uint32_t *>(ring);
        for (int32_t v = lane; v < n_vec; v += 64) {
            const int32_t s = body + 16 * v;
            const uint32_t sh = 8u * (uint32_t) (s & 3);
            uint32_t w[5];
            for (int k = 0; k < 5; k++) w[k] = ring32[(uint32_t) ((s >> 2) + k) & (kRing / 4 - 1)];
            uint4 q;
            q.x = (uint32_t) ((((uint64_t) w[1] << 32) | w[0]) >> sh);
            q.y = (uint32_t) ((((uint64_t) w[2] << 32) | w[1]) >> sh);
            q.z = (uint32_t) ((((uint64_t) w[3] << 32) | w[2]) >> sh);
            q.w = (uint32_t) ((((uint64_t) w[4] << 32) | w[3]) >> sh);
            *reinterpret_cast<uint4 *>(dst + (s - skip)) = q;
        }
        const int32_t tail = body + 16 * n_vec;
        if (tail + lane < hi) dst[tail - skip + lane] = ring[(tail + lane) & (kRing - 1)];
    }
    __device__ __forceinline__ void ensure_out(int32_t pos, int32_t k)
    {
        if (pos + k - flushed > kRing) flush(pos);
    }
    __device__ __forceinline__ void stored(int32_t src, int32_t len, int32_t pos)
    {
        while (len > 0) {
            if (pos - flushed >= kRing) flush(pos);
            int32_t chunk = kRing - (pos - flushed);
            if (chunk > len) chunk = len;
            for (int32_t i = lane; i < chunk; i += 64) ring[(pos + i) & (kRing - 1)] = comp[abs0 + src + i];
            fence();
            src += chunk; pos += chunk; len -= chunk;
        }
    }
    __device__ __forceinline__ void finish(int32_t pos) { flush(pos); }
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *__restrict__ comp, int64_t comp_cap,
                                                     const dn::InflateBlock *__restrict__ blk, int64_t n_blocks,
                                                     uint8_t *__restrict__ out, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[kRing];
    __shared__ __attribute__((aligned(16))) uint32_t s_win[kWin / 4];
    __shared__ uint16_t s_lit[1 << kLitBits], s_dist[1 << kDistBits], s_sym_l[288], s_sym_d[32], s_cnt_l[16], s_cnt_d[16], s_offs[16];
    __shared__ uint8_t s_lens[320];
    const int64_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const dn::InflateBlock B = blk[b];
    Tables t{s_lit, s_dist, s_sym_l, s_sym_d, s_cnt_l, s_cnt_d, s_offs, s_lens};
    WaveMem m;
    m.ring = s_ring;
    m.win = s_win;
    m.comp = comp;
    m.comp_cap = comp_cap;
    m.abs0 = B.pay_off;
    m.wbase = -4 * (int64_t) kWin;
    m.dst = out + B.dst_off;
    m.skip = B.skip;
    m.keep = B.keep;
    m.flushed = 0;
    m.lane = (int) threadIdx.x;
    m.check = B.check != 0;
    m.crc = 0xffffffffu;
    const int rc = inflate_block(m, t, B.pay_len, B.isize, B.crc);
    if (threadIdx.x == 0) status[b] = rc;
}

int bad(const std::string &msg) { return dn::fail(DN_E_INVALID, msg); }

// the checks of the entry points; fills blk (skip 0, output at out_off[b]; out == nullptr, where the entry point allows it:
// nothing kept).  crc32 (nullable): the CRC32 every block must have.
int validate(const char *who, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
             const int64_t *out_off, const uint8_t *out, bool out_optional, const int32_t *status, const uint32_t *crc32,
             std::vector<dn::InflateBlock> &blk)
{
    const std::string w(who);
    if (n_comp < 0 || n_blocks < 0 || (n_comp > 0 && !comp) || !out_off || (n_blocks > 0 && (!pay_off || !pay_len || !status)))
        return bad(w + ": bad argument");
    if (out_off[0] != 0) return bad(w + ": out_off[0] is not 0");
    blk.resize((size_t) n_blocks);
    for (int64_t b = 0; b < n_blocks; b++) {
        const int64_t isize = out_off[b + 1] - out_off[b];
        if (!dn::payload_inside(pay_off[b], pay_len[b], n_comp)) return bad(w + ": payload of block " + std::to_string(b) + " outside comp");
        if (isize < 0 || isize > 65536) return bad(w + ": block " + std::to_string(b) + " has an inflated size outside 0 .. 65536");
        blk[(size_t) b] = dn::InflateBlock{pay_off[b], out ? out_off[b] : 0, pay_len[b], (int32_t) isize, 0, out ? (int32_t) isize : 0,
                                           crc32 ? crc32[b] : 0u, crc32 ? 1 : 0};
    }
    if (out_off[n_blocks] > 0 && !out && !out_optional) return bad(w + ": bad argument");
    return DN_OK;
}

int inflate_host(const char *who, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                 const int64_t *out_off, uint8_t *out, bool out_optional, int32_t *status, const uint32_t *crc32)
{
    dn::clear_error();
    std::vector<dn::InflateBlock> blk;
    const int rc = validate(who, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, out_optional, status, crc32, blk);
    if (rc != DN_OK) return rc;
    uint16_t lit[1 << kLitBits], dist[1 << kDistBits], sym_l[288], sym_d[32], cnt_l[16], cnt_d[16], offs[16];
    uint8_t lens[320];
    const Tables t{lit, dist, sym_l, sym_d, cnt_l, cnt_d, offs, lens};
    std::vector<uint8_t> dropped(out ? 0 : 65536);
    for (const dn::InflateBlock &B : blk) {
        HostMem m{comp + B.pay_off, out ? out + B.dst_off : dropped.data(), B.check != 0};
        status[&B - blk.data()] = inflate_block(m, t, B.pay_len, B.isize, B.crc);
    }
    return DN_OK;
}

int inflate_device(const char *who, int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                   const int32_t *pay_len, const int64_t *out_off, uint8_t *out, bool out_optional, int32_t *status, double *copy_ms,
                   double *device_ms, const uint32_t *crc32)
{
    dn::clear_error();
    std::vector<dn::InflateBlock> blk;
    const int rc = validate(who, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, out_optional, status, crc32, blk);
    if (rc != DN_OK) return rc;
    if (copy_ms) *copy_ms = 0.0;
    if (device_ms) *device_ms = 0.0;
    if (n_blocks == 0) return DN_OK;
    if (n_blocks > INT32_MAX) return bad(std::string(who) + ": too many blocks");
    const int64_t n_out = out ? out_off[n_blocks] : 0, cap = dn::inflate_comp_cap(n_comp);
    dn::Stream st;
    dn::Event e0, e1, e2;
    dn::DeviceBuffer<uint8_t> d_comp, d_out;
    dn::DeviceBuffer<dn::InflateBlock> d_blk;
    dn::DeviceBuffer<int32_t> d_status;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate)); DN_TRY(e1.create(hipEventCreate)); DN_TRY(e2.create(hipEventCreate));
        DN_TRY(d_comp.alloc((size_t) cap));
        DN_TRY(d_out.alloc((size_t) n_out + 16));
        DN_TRY(d_blk.alloc(sizeof(dn::InflateBlock) * (size_t) n_blocks));
        DN_TRY(d_status.alloc(sizeof(int32_t) * (size_t) n_blocks));
        DN_TRY(hipEventRecord(e0, st));
        if (n_comp > 0) DN_TRY(hipMemcpyAsync(d_comp, comp, (size_t) n_comp, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_blk, blk.data(), sizeof(dn::InflateBlock) * (size_t) n_blocks, hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));
        DN_TRY(dn::inflate_launch(st, d_comp, cap, d_blk, n_blocks, d_out, d_status));
        DN_TRY(hipEventRecord(e2, st));
        if (n_out > 0) DN_TRY(hipMemcpyAsync(out, d_out, (size_t) n_out, hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t) n_blocks, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        float ms = 0.f;
        if (copy_ms) { DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *copy_ms = ms; }
        if (device_ms) { DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *device_ms = ms; }
        return DN_OK;
    });
}

}  // namespace

hipError_t dn::inflate_launch(hipStream_t st, const uint8_t *d_comp, int64_t comp_cap, const InflateBlock *d_blk, int64_t n_blocks,
                              uint8_t *d_out, int32_t *d_status)
{
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned) n_blocks), dim3(64), 0, st, d_comp, comp_cap, d_blk, n_blocks, d_out, d_status);
    return hipGetLastError();
}

int dn::InflateWindow::arm(const char *who, const uint32_t *crc32, int64_t n_blocks)
{
    if (n_blocks < 0 || n_blocks > INT32_MAX || (n_blocks > 0 && !crc32)) return bad(std::string(who) + ": bad argument");
    announced.assign(crc32, crc32 + n_blocks);
    armed = true;
    return DN_OK;
}

int dn::InflateWindow::plan(const char *who, const char *armed_by, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                            const int32_t *pay_len, const int32_t *isize, int32_t head_skip, int32_t tail_keep, int64_t base, int64_t &total)
{
    const std::string w(who);
    if (checking && (int64_t) crc.size() != n_blocks)
        return bad(w + ": " + std::to_string(crc.size()) + " CRC32s were announced (" + armed_by + ") for " + std::to_string(n_blocks) + " blocks");
    blk.resize((size_t) n_blocks);
    total = base;
    for (int64_t b = 0; b < n_blocks; b++) {
        if (isize[b] < 0) return bad(w + ": block " + std::to_string(b) + " has a negative inflated size");
        if (!payload_inside(pay_off[b], pay_len[b], n_comp)) return bad(w + ": payload of block " + std::to_string(b) + " outside comp");
        int32_t skip, keep;
        window_trim(b, n_blocks, isize[b], head_skip, tail_keep, skip, keep);
        blk[(size_t) b] = InflateBlock{pay_off[b], total, pay_len[b], isize[b], skip, keep, checking ? crc[(size_t) b] : 0u, checking ? 1 : 0};
        total += keep;
    }
    return DN_OK;
}

int dn::InflateWindow::queue(hipStream_t st, const uint8_t *comp_bytes, int64_t n_comp, uint8_t *d_out, int32_t *status)
{
    const int64_t n_blocks = (int64_t) blk.size(), comp_cap = inflate_comp_cap(n_comp);
    DN_TRY(comp.reserve(comp_cap, 0, st));
    DN_TRY(d_blk.reserve(n_blocks, 0, st)); DN_TRY(d_status.reserve(n_blocks, 0, st));
    if (!ev0) { DN_TRY(ev0.create(hipEventCreate)); DN_TRY(ev1.create(hipEventCreate)); }
    if (n_comp > 0) DN_TRY(hipMemcpyAsync(comp, comp_bytes, (size_t) n_comp, hipMemcpyHostToDevice, st));
    if (n_blocks > 0) DN_TRY(hipMemcpyAsync(d_blk, blk.data(), sizeof(InflateBlock) * (size_t) n_blocks, hipMemcpyHostToDevice, st));
    DN_TRY(hipEventRecord(ev0, st));
    DN_TRY(inflate_launch(st, comp, comp_cap, d_blk, n_blocks, d_out, d_status));
    DN_TRY(hipEventRecord(ev1, st));
    if (n_blocks > 0) DN_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t) n_blocks, hipMemcpyDeviceToHost, st));
    return DN_OK;
}

int dn::InflateWindow::wait(hipStream_t st, const int32_t *status, double *ms, bool &ok)
{
    DN_TRY(hipStreamSynchronize(st));
    if (ms) {
        float t = 0.f;
        DN_TRY(hipEventElapsedTime(&t, ev0, ev1));
        *ms = t;
    }
    ok = true;
    for (size_t b = 0; b < blk.size(); b++) ok = ok && status[b] == 0;
    return DN_OK;
}

extern "C" int dn_bgzf_inflate_host(const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                                    const int64_t *out_off, uint8_t *out, int32_t *status)
{
    return inflate_host("dn_bgzf_inflate_host", comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, false, status, nullptr);
}

extern "C" int dn_bgzf_inflate_check_host(const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                                          const int64_t *out_off, uint8_t *out, int32_t *status, const uint32_t *crc32)
{
    return inflate_host("dn_bgzf_inflate_check_host", comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, true, status, crc32);
}

extern "C" int dn_bgzf_inflate(int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                               const int32_t *pay_len, const int64_t *out_off, uint8_t *out, int32_t *status, double *copy_ms,
                               double *device_ms)
{
    return inflate_device("dn_bgzf_inflate", device, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, false, status, copy_ms, device_ms,
                          nullptr);
}

extern "C" int dn_bgzf_inflate_check(int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                                     const int32_t *pay_len, const int64_t *out_off, uint8_t *out, int32_t *status, double *copy_ms,
                                     double *device_ms, const uint32_t *crc32)
{
    return inflate_device("dn_bgzf_inflate_check", device, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, true, status, copy_ms,
                          device_ms, crc32);
}

extern "C" int dn_bgzf_crc32_host(const uint8_t *data, int64_t n, int32_t lanes, int32_t flush_bytes, uint32_t *crc)
{
    dn::clear_error();
    if (n < 0 || (n > 0 && !data) || lanes < 1 || lanes > 64 || flush_bytes < 1 || flush_bytes > (1 << 30) || !crc)
        return bad("dn_bgzf_crc32_host: bad argument (lanes is 1 .. 64, flush_bytes 1 .. 2^30)");
    *crc = crc_host(0xffffffffu, data, n, lanes, flush_bytes) ^ 0xffffffffu;
    return DN_OK;
}

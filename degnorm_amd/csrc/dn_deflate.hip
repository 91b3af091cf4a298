// dn_deflate.hip -- raw DEFLATE (RFC 1951) encoder that writes whole BGZF blocks, one block per wavefront.
//
// The counterpart of dn_inflate.hip and written the same way: the encoder (deflate_block) is __host__ __device__ code against
// a memory policy M.
//
//   HostDef   one lane: every "for (i = lane; i < n; i += kLanes)" loop below runs serially.  What dn_bgzf_deflate_host runs,
//             block after block, without a device.
//   WaveDef   one 64-lane workgroup (one wave) per BGZF block, everything but the input in LDS (47.8 KiB: three workgroups
//             per CU).  Parallel steps are lane-strided loops; serial steps run in lane 0 between wavefront fences.
//
// Both builds write the same bytes for every input, because nothing below depends on the order in which lanes act: the
// parse is defined per step of 64 positions against the hash table as it stood before the step, the table then takes the
// largest position per hash (max is order-free), histograms are sums, the bits of a token go to a place given by a prefix
// sum, and they are or-ed into zeroed memory.  DESIGN.md ("BGZF deflate") has the definition and the size bound.
//
// A BGZF block holds len <= 0xff00 input bytes.  They are cut into DEFLATE blocks by position: DEFLATE block k holds the
// tokens that start in [k * kCut, (k + 1) * kCut); the history of matches spans the whole BGZF block.  Per DEFLATE block:
// parse (tokens in LDS), histograms, code lengths (Huffman on rank-sorted frequencies, limited to 15 / 7 bits), the exact
// size of the dynamic, fixed and stored forms, and the smallest is emitted into an LDS staging area that is written out in
// 16-byte stores.  So no DEFLATE block is larger than its stored form and a BGZF block never exceeds dn::deflate_bound.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_deflate.hpp"

#define DN_HD __host__ __device__ __forceinline__
#include "dn_crc.hpp"

namespace {

constexpr int kHashBits = 12, kHash = 1 << kHashBits;   // entries of the table of most recent positions
constexpr int kCut = 8192;                               // input positions per DEFLATE block
constexpr int kStep = 64;                                // positions parsed against one state of the table
constexpr int kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr int kStage = kCut + 512;                       // bytes of staging: a carried 16-byte piece and a block's stored form
constexpr int kLit = 0, kDist = 288, kCl = 320, kSyms = 340;   // where the three alphabets lie in freq / lens / code
constexpr uint32_t kNoHash = 0xffffu;
constexpr int kHeadBytes = 18;
enum { kStored = 0, kFixed = 1, kDynamic = 2 };
enum { mHlit = 0, mHdist, mNcls, mHclen, mKind, mBits, mCount };

static_assert(kCut % kStep == 0 && kCut > kMaxMatch, "a DEFLATE block holds whole steps and at least one token");
static_assert(dn::kDeflateMaxLen + 26 + 6 * ((dn::kDeflateMaxLen + kCut - 1) / kCut) + 32 <= dn::kDeflateSlot, "a block and the reads behind it fit its slot");

struct Work {
    uint32_t *hash;                  // kHash: position + 1 of the latest 4 bytes with this hash, 0 = none
    uint16_t *tok;                   // kCut slots: a literal (0 .. 255), or 256 + (length - 3) followed by 0x8000 | (distance - 1)
    uint32_t *stage;                 // kStage / 4 words: output bytes from byte `sbase` of the block on
    uint16_t *mlen, *mdist, *mhash;  // kStep each: per position of the step the match (length or 0; distance - 1 or the literal) and its hash
    uint32_t *freq;                  // kSyms
    uint8_t *lens;                   // kSyms
    uint16_t *code;                  // kSyms: the codes, bit-reversed
    uint16_t *cls;                   // 320: the code-length symbols of a dynamic header, symbol | extra << 5
    uint16_t *srt;                   // 288: used symbols by ascending (frequency, symbol)
    uint32_t *wt;                    // 576: weights of the leaves (sorted) and the internal nodes of the Huffman tree
    uint16_t *par;                   // 576: parent of each node, then its depth
    uint32_t *blc;                   // 32: codes per length, next code per length
    uint32_t *misc;                  // mCount values lane 0 hands to the wave
};

DN_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

DN_HD uint32_t rev_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// length - 3 (0 .. 255) and distance - 1 (0 .. 32767) -> symbol, number of extra bits and their value (RFC 1951, 3.2.5)
DN_HD void len_symbol(uint32_t l, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
    if (l == 255) { sym = 285; eb = 0; ev = 0; return; }
    const uint32_t e = (uint32_t) (31 - __builtin_clz(l)) - 2;
    sym = 261 + 4 * e + ((l >> e) & 3u); eb = e; ev = l & ((1u << e) - 1u);
}
DN_HD void dist_symbol(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    if (d < 4) { sym = d; eb = 0; ev = 0; return; }
    const uint32_t e = (uint32_t) (31 - __builtin_clz(d)) - 1;
    sym = 2 * e + 2 + ((d >> e) & 1u); eb = e; ev = d & ((1u << e) - 1u);
}
DN_HD uint32_t len_extra(uint32_t s) { return s < 265 || s >= 285 ? 0u : (s - 261) >> 2; }
DN_HD uint32_t dist_extra(uint32_t d) { return d < 4 ? 0u : (d - 2) >> 1; }
DN_HD uint32_t fixed_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// v (at most 48 bits) or-ed into the staging words from bit `rel` of the staging area on
template <class M> DN_HD void put_bits(M &m, uint32_t *stage, int32_t rel, uint64_t v)
{
    const int32_t k = rel >> 5;
    const uint32_t sh = (uint32_t) rel & 31u, lo = (uint32_t) v, hi = (uint32_t) (v >> 32);
    const uint32_t w0 = lo << sh, w1 = (sh ? lo >> (32 - sh) : 0u) | (hi << sh), w2 = sh ? hi >> (32 - sh) : 0u;
    if (w0) m.orw(stage + k, w0);
    if (w1) m.orw(stage + k + 1, w1);
    if (w2) m.orw(stage + k + 2, w2);
}

// how many bytes of the input agree from positions c and p on, at most maxl
template <class M> DN_HD uint32_t match_len(M &m, int32_t c, int32_t p, int32_t maxl)
{
    int32_t k = 0;
    while (k + 4 <= maxl) {
        const uint32_t x = m.in4(c + k) ^ m.in4(p + k);
        if (x) return (uint32_t) (k + (__builtin_ctz(x) >> 3));
        k += 4;
    }
    while (k < maxl && m.in(c + k) == m.in(p + k)) k++;
    return (uint32_t) k;
}

// The serial part of build_lengths: lens[0 .. n) of a complete prefix code of at most `limit` bits for the used symbols,
// which w.srt holds by ascending (frequency, symbol).  Huffman's algorithm with two queues; a tree deeper than the limit
// has its deep leaves moved to the limit and the excess of the Kraft sum taken back one leaf at a time.
DN_HD void lengths_serial(const Work &w, const uint32_t *freq, int n, int limit, uint8_t *lens)
{
    int u = 0;
    for (int i = 0; i < n; i++) u += freq[i] != 0 ? 1 : 0;
    if (u == 0) return;
    if (u == 1) { lens[w.srt[0]] = 1; return; }
    for (int k = 0; k < u; k++) w.wt[k] = freq[w.srt[k]];
    int a = 0, b = u;
    for (int nn = u; nn < 2 * u - 1; nn++) {            // leaves wait in [a, u), internal nodes in [b, nn); a leaf wins a tie
        uint32_t sum = 0;
        for (int t = 0; t < 2; t++) {
            int x;
            if (a < u && (b >= nn || w.wt[a] <= w.wt[b])) x = a++;
            else x = b++;
            sum += w.wt[x];
            w.par[x] = (uint16_t) nn;
        }
        w.wt[nn] = sum;
    }
    w.par[2 * u - 2] = 0;                                // the root's depth; parents have larger indices than their children
    for (int x = 2 * u - 3; x >= 0; x--) w.par[x] = (uint16_t) (w.par[w.par[x]] + 1);
    for (int l = 0; l < 16; l++) w.blc[l] = 0;
    for (int k = 0; k < u; k++) { const int d = w.par[k] > limit ? limit : w.par[k]; w.blc[d] = w.blc[d] + 1; }
    int32_t excess = -(1 << limit);                      // Kraft sum - 1, in units of 2^-limit
    for (int l = 1; l <= limit; l++) excess += (int32_t) (w.blc[l] << (limit - l));
    while (excess > 0) {                                 // the deepest leaf above the limit goes one level down
        int l = limit - 1;
        while (w.blc[l] == 0) l--;
        w.blc[l] = w.blc[l] - 1; w.blc[l + 1] = w.blc[l + 1] + 1;
        excess -= 1 << (limit - l - 1);
    }
    while (excess < 0) {                                 // overshot: the deepest leaf whose gain still fits goes one level up
        int l = limit;
        while (w.blc[l] == 0 || (1 << (limit - l)) > -excess) l--;
        w.blc[l] = w.blc[l] - 1; w.blc[l - 1] = w.blc[l - 1] + 1;
        excess += 1 << (limit - l);
    }
    int k = 0;
    for (int l = limit; l >= 1; l--)
        for (uint32_t c = 0; c < w.blc[l]; c++) lens[w.srt[k++]] = (uint8_t) l;
}

template <class M> DN_HD void build_lengths(M &m, const Work &w, const uint32_t *freq, int n, int limit, uint8_t *lens)
{
    for (int i = m.lane; i < n; i += M::kLanes) {       // rank sort: every used symbol counts those before it
        const uint32_t f = freq[i];
        if (f) {
            int r = 0;
            for (int j = 0; j < n; j++) { const uint32_t g = freq[j]; r += (g != 0 && (g < f || (g == f && j < i))) ? 1 : 0; }
            w.srt[r] = (uint16_t) i;
        }
        lens[i] = 0;
    }
    m.fence();
    if (m.lane == 0) lengths_serial(w, freq, n, limit, lens);
    m.fence();
}

// canonical codes of lens[0 .. n), bit-reversed for a writer that starts at the lowest bit
DN_HD void assign_codes(const Work &w, const uint8_t *lens, int n, uint16_t *code)
{
    for (int l = 0; l < 16; l++) w.blc[l] = 0;
    for (int i = 0; i < n; i++) w.blc[lens[i]] = w.blc[lens[i]] + 1;
    uint32_t c = 0;
    w.blc[0] = 0;
    for (int l = 1; l < 16; l++) { c = (c + w.blc[l - 1]) << 1; w.blc[16 + l] = c; }
    for (int i = 0; i < n; i++) {
        const int l = lens[i];
        if (l) { code[i] = (uint16_t) rev_bits(w.blc[16 + l], l); w.blc[16 + l] = w.blc[16 + l] + 1; }
        else code[i] = 0;
    }
}

// lane 0, after the literal/length and distance lengths are known: HLIT, HDIST and the run-length form of the lengths
// (16: the length before, 3 .. 6 times; 17: 3 .. 10 zeros; 18: 11 .. 138 zeros), with the histogram of its symbols
DN_HD void plan_header(const Work &w)
{
    int hlit = 286, hdist = 30;
    while (hlit > 257 && w.lens[kLit + hlit - 1] == 0) hlit--;
    while (hdist > 1 && w.lens[kDist + hdist - 1] == 0) hdist--;
    for (int k = 0; k < 19; k++) w.freq[kCl + k] = 0;
    const int total = hlit + hdist;
    int i = 0, nc = 0;
    const auto at = [&](int j) { return (int) w.lens[j < hlit ? kLit + j : kDist + j - hlit]; };
    const auto emit = [&](int sym, int extra) { w.cls[nc++] = (uint16_t) (sym | extra << 5); w.freq[kCl + sym] = w.freq[kCl + sym] + 1; };
    while (i < total) {
        const int v = at(i);
        int run = 1;
        while (i + run < total && at(i + run) == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; emit(18, r - 11); run -= r; }
            if (run >= 3) { emit(17, run - 3); run = 0; }
        } else {
            emit(v, 0); run--;
            while (run >= 3) { const int r = run < 6 ? run : 6; emit(16, r - 3); run -= r; }
        }
        for (; run > 0; run--) emit(v, 0);
    }
    int used = 0, one = 0;
    for (int k = 0; k < 19; k++)
        if (w.freq[kCl + k]) { used++; one = k; }
    if (used == 1) w.freq[kCl + (one == 0 ? 1 : 0)] = 1;         // the code-length code must be complete: a second, unused code
    w.misc[mHlit] = (uint32_t) hlit; w.misc[mHdist] = (uint32_t) hdist; w.misc[mNcls] = (uint32_t) nc;
}

// lane 0, after the code-length code's lengths are known: the exact sizes of the three forms of the DEFLATE block that
// holds the histograms' tokens and `raw` input bytes, the choice, the codes of the chosen form and the block's header.
// rel: where the block starts in the staging area, in bits; misc[mBits] = the bits written.
template <class M> DN_HD void choose_and_head(M &m, const Work &w, int32_t rel, int32_t raw, bool last)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int hlit = (int) w.misc[mHlit], hdist = (int) w.misc[mHdist], nc = (int) w.misc[mNcls];
    int hclen = 19;
    while (hclen > 4 && w.lens[kCl + order[hclen - 1]] == 0) hclen--;
    uint32_t body_d = 0, body_f = 0;
    for (uint32_t s = 0; s < 286; s++) {
        const uint32_t f = w.freq[kLit + s];
        body_d += f * (w.lens[kLit + s] + len_extra(s));
        body_f += f * (fixed_len(s) + len_extra(s));
    }
    for (uint32_t d = 0; d < 30; d++) {
        const uint32_t f = w.freq[kDist + d];
        body_d += f * (w.lens[kDist + d] + dist_extra(d));
        body_f += f * (5 + dist_extra(d));
    }
    uint32_t head_d = 3 + 14 + 3 * (uint32_t) hclen;
    for (int k = 0; k < nc; k++) {
        const uint32_t s = w.cls[k] & 31u;
        head_d += w.lens[kCl + s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
    }
    const uint32_t pad = (8u - (((uint32_t) rel + 3u) & 7u)) & 7u;
    const uint32_t dyn = head_d + body_d, fix = 3 + body_f, sto = 3 + pad + 32 + 8 * (uint32_t) raw;
    const int kind = dyn < fix && dyn < sto ? kDynamic : fix < sto ? kFixed : kStored;
    w.misc[mKind] = (uint32_t) kind;
    int32_t at = rel;
    put_bits(m, w.stage, at, (uint64_t) ((last ? 1u : 0u) | (uint32_t) kind << 1));
    at += 3;
    if (kind == kStored) {
        at += (int32_t) pad;
        put_bits(m, w.stage, at, (uint64_t) ((uint32_t) raw | ((~(uint32_t) raw & 0xffffu) << 16)));
        at += 32;
    } else if (kind == kFixed) {
        for (uint32_t s = 0; s < 288; s++) w.lens[kLit + s] = (uint8_t) fixed_len(s);
        for (uint32_t d = 0; d < 32; d++) w.lens[kDist + d] = 5;
        assign_codes(w, w.lens + kLit, 288, w.code + kLit);
        assign_codes(w, w.lens + kDist, 32, w.code + kDist);
    } else {
        assign_codes(w, w.lens + kLit, 286, w.code + kLit);
        assign_codes(w, w.lens + kDist, 30, w.code + kDist);
        assign_codes(w, w.lens + kCl, 19, w.code + kCl);
        put_bits(m, w.stage, at, (uint64_t) ((uint32_t) (hlit - 257) | (uint32_t) (hdist - 1) << 5 | (uint32_t) (hclen - 4) << 10));
        at += 14;
        for (int k = 0; k < hclen; k++) { put_bits(m, w.stage, at, (uint64_t) w.lens[kCl + order[k]]); at += 3; }
        for (int k = 0; k < nc; k++) {
            const uint32_t s = w.cls[k] & 31u, x = (uint32_t) w.cls[k] >> 5, l = w.lens[kCl + s];
            const uint32_t xb = s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u;
            put_bits(m, w.stage, at, (uint64_t) (w.code[kCl + s] | x << l));
            at += (int32_t) (l + xb);
        }
    }
    w.misc[mBits] = (uint32_t) (at - rel);
}

// One BGZF block of the len input bytes the policy reaches; returns its size.  All of it goes through the staging area:
// stage word j holds bytes sbase + 4 j .. of the block, sbase a multiple of 16, and complete 16-byte pieces leave after
// every DEFLATE block.
template <class M> DN_HD int32_t deflate_block(M &m, const Work &w, int32_t len)
{
    const int lane = m.lane;
    for (int i = lane; i < kHash; i += M::kLanes) w.hash[i] = 0;
    for (int i = lane; i < kStage / 4; i += M::kLanes) w.stage[i] = 0;
    m.fence();
    if (lane == 0) { w.stage[0] = 0x04088b1fu; w.stage[2] = 0x0006ff00u; w.stage[3] = 0x00024342u; }     // BSIZE is patched at the end
    m.fence();
    int32_t bitpos = 8 * kHeadBytes, sbase = 0, next = 0;

    // complete 16-byte pieces (all of them when `last`) -> the output; the piece in progress moves to the front
    const auto flush = [&](bool last) {
        m.fence();
        const int32_t bytes = (last ? (bitpos + 7) >> 3 : bitpos >> 3) - sbase, n = last ? (bytes + 15) >> 4 : bytes >> 4;
        for (int32_t j = lane; j < n; j += M::kLanes) m.store16(sbase + 16 * j, w.stage + 4 * j);
        m.fence();
        if (last || n == 0) return;
        const int32_t used = ((bitpos + 31) >> 5) - (sbase >> 2) + 1;
        for (int32_t k = lane; k < 4; k += M::kLanes) w.stage[k] = w.stage[4 * n + k];
        m.fence();
        for (int32_t k = 4 + lane; k < used; k += M::kLanes) w.stage[k] = 0;
        m.fence();
        sbase += 16 * n;
    };

    for (int32_t base = 0; base == 0 || next < len; base += kCut) {
        const int32_t start = next, cut = len < base + kCut ? len : base + kCut;
        int32_t n_slots = 0;
        for (int i = lane; i < kCl; i += M::kLanes) w.freq[i] = 0;
        m.fence();
        // --- parse: the tokens that start in [start, cut)
        for (int32_t p0 = base; p0 < cut; p0 += kStep) {
            for (int i = lane; i < kStep; i += M::kLanes) {
                const int32_t p = p0 + i;
                uint32_t ml = 0, md = 0, h = kNoHash;
                if (p + 4 <= len) {
                    h = hash4(m.in4(p));
                    const uint32_t e = w.hash[h];
                    if (p >= next && e != 0 && p - (int32_t) (e - 1) <= kMaxDist) {
                        const int32_t c = (int32_t) e - 1, room = len - p;
                        ml = match_len(m, c, p, room < kMaxMatch ? room : kMaxMatch);
                        md = (uint32_t) (p - c - 1);
                    }
                }
                if (ml < (uint32_t) kMinMatch) { ml = 0; md = p < len ? m.in(p) : 0u; }
                w.mlen[i] = (uint16_t) ml; w.mdist[i] = (uint16_t) md; w.mhash[i] = (uint16_t) h;
            }
            m.fence();
            for (int i = lane; i < kStep; i += M::kLanes) {
                const uint32_t h = w.mhash[i];
                if (h != kNoHash) m.hmax(w.hash + h, (uint32_t) (p0 + i + 1));
            }
            if (lane == 0) {                                    // greedy, from the first position no match covers
                int32_t q = next > p0 ? next : p0, ns = n_slots;
                const int32_t end = p0 + kStep < cut ? p0 + kStep : cut;
                while (q < end) {
                    const int32_t i = q - p0, ml = w.mlen[i];
                    if (ml) {
                        w.tok[ns++] = (uint16_t) (256 + ml - 3);
                        w.tok[ns++] = (uint16_t) (0x8000u | w.mdist[i]);
                        q += ml;
                    } else {
                        w.tok[ns++] = w.mdist[i];
                        q++;
                    }
                }
                next = q; n_slots = ns;
            }
            next = m.bcast(next); n_slots = m.bcast(n_slots);
            m.fence();
        }
        const bool last = next >= len;
        // --- histograms and code lengths
        for (int32_t i = lane; i < n_slots; i += M::kLanes) {
            const uint32_t t = w.tok[i];
            uint32_t sym, eb, ev;
            if (t & 0x8000u) { dist_symbol(t & 0x7fffu, sym, eb, ev); m.add(w.freq + kDist + sym, 1u); }
            else if (t < 256) m.add(w.freq + kLit + t, 1u);
            else { len_symbol(t - 256, sym, eb, ev); m.add(w.freq + kLit + sym, 1u); }
        }
        if (lane == 0) w.freq[kLit + 256] = 1;
        m.fence();
        build_lengths(m, w, w.freq + kLit, 286, 15, w.lens + kLit);
        build_lengths(m, w, w.freq + kDist, 30, 15, w.lens + kDist);
        if (lane == 0) plan_header(w);
        m.fence();
        build_lengths(m, w, w.freq + kCl, 19, 7, w.lens + kCl);
        if (lane == 0) choose_and_head(m, w, bitpos - 8 * sbase, next - start, last);
        m.fence();
        const int kind = (int) w.misc[mKind];
        bitpos += (int32_t) w.misc[mBits];
        // --- the block's body
        if (kind == kStored) {
            uint8_t *bytes = reinterpret_cast<uint8_t *>(w.stage) + ((bitpos >> 3) - sbase);
            for (int32_t i = lane; i < next - start; i += M::kLanes) bytes[i] = (uint8_t) m.in(start + i);
            bitpos += 8 * (next - start);
        } else {
            for (int32_t i0 = 0; i0 < n_slots; i0 += M::kLanes) {
                const int32_t i = i0 + lane;
                uint64_t v = 0;
                int32_t nb = 0;
                if (i < n_slots) {
                    const uint32_t t = w.tok[i];
                    if (t < 256) { v = w.code[kLit + t]; nb = w.lens[kLit + t]; }
                    else if (!(t & 0x8000u)) {
                        uint32_t sym, eb, ev;
                        len_symbol(t - 256, sym, eb, ev);
                        v = (uint64_t) w.code[kLit + sym] | (uint64_t) ev << w.lens[kLit + sym];
                        nb = (int32_t) (w.lens[kLit + sym] + eb);
                        dist_symbol(w.tok[i + 1] & 0x7fffu, sym, eb, ev);
                        v |= (uint64_t) w.code[kDist + sym] << nb;
                        nb += w.lens[kDist + sym];
                        v |= (uint64_t) ev << nb;
                        nb += (int32_t) eb;
                    }
                }
                int32_t total = 0;
                const int32_t off = m.scan(nb, total);
                if (nb) put_bits(m, w.stage, bitpos - 8 * sbase + off, v);
                bitpos += total;
            }
            m.fence();
            if (lane == 0) put_bits(m, w.stage, bitpos - 8 * sbase, (uint64_t) w.code[kLit + 256]);
            bitpos += w.lens[kLit + 256];
        }
        flush(false);
    }
    // --- the trailer
    const uint32_t crc = m.crc(len);
    bitpos = (bitpos + 7) & ~7;
    if (lane == 0) put_bits(m, w.stage, bitpos - 8 * sbase, (uint64_t) crc);
    if (lane == 0) put_bits(m, w.stage, bitpos - 8 * sbase + 32, (uint64_t) (uint32_t) len);
    bitpos += 64;
    flush(true);
    m.bsize((uint32_t) ((bitpos >> 3) - 1));
    return bitpos >> 3;
}

// --- host: one lane, plain arrays -------------------------------------------------------------------------------------------

struct HostDef {
    static constexpr int kLanes = 1;
    const uint8_t *src;             // the block's input
    uint8_t *dst;                   // dn::kDeflateSlot bytes
    int lane = 0;

    void fence() {}
    uint32_t in(int32_t p) const { return src[p]; }
    uint32_t in4(int32_t p) const { uint32_t v; memcpy(&v, src + p, 4); return v; }
    void hmax(uint32_t *a, uint32_t v) { if (v > *a) *a = v; }
    void add(uint32_t *a, uint32_t v) { *a += v; }
    void orw(uint32_t *a, uint32_t v) { *a |= v; }
    int32_t scan(int32_t v, int32_t &total) { total = v; return 0; }
    int32_t bcast(int32_t v) { return v; }
    void store16(int32_t off, const uint32_t *w) { memcpy(dst + off, w, 16); }
    void bsize(uint32_t v) { dst[16] = (uint8_t) v; dst[17] = (uint8_t) (v >> 8); }
    uint32_t crc(int32_t len) const { return crc_host(0xffffffffu, src, len, 64, 32768) ^ 0xffffffffu; }
};

struct HostWork {
    uint32_t hash[kHash], stage[kStage / 4], freq[kSyms], wt[576], blc[32], misc[mCount];
    uint16_t tok[kCut], mlen[kStep], mdist[kStep], mhash[kStep], code[kSyms], cls[320], srt[288], par[576];
    uint8_t lens[kSyms];
    Work work() { return Work{hash, tok, stage, mlen, mdist, mhash, freq, lens, code, cls, srt, wt, par, blc, misc}; }
};

// --- device: one wave, everything but the input in LDS ---------------------------------------------------------------------

struct GlobalReader {                                               // crc_slice's view of the input: dwords of the array the block lies in
    const uint32_t *d32;
    __device__ __forceinline__ uint32_t dword(int32_t p) const { return d32[p >> 2]; }
};

struct WaveDef {
    static constexpr int kLanes = 64;
    const uint8_t *src;             // the block's input
    const uint32_t *src32;          // the dword that holds its first byte, which is byte `mis` of it
    int32_t mis;
    uint8_t *dst;                   // the block's slot, 16-byte aligned
    int lane;

    __device__ __forceinline__ void fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
    __device__ __forceinline__ uint32_t in(int32_t p) const { return src[p]; }
    __device__ __forceinline__ uint32_t in4(int32_t p) const { uint32_t v; __builtin_memcpy(&v, src + p, 4); return v; }
    __device__ __forceinline__ void hmax(uint32_t *a, uint32_t v) { atomicMax(a, v); }
    __device__ __forceinline__ void add(uint32_t *a, uint32_t v) { atomicAdd(a, v); }
    __device__ __forceinline__ void orw(uint32_t *a, uint32_t v) { atomicOr(a, v); }
    __device__ __forceinline__ int32_t scan(int32_t v, int32_t &total)      // exclusive sum over the wave
    {
        int32_t s = v;
        for (int o = 1; o < 64; o <<= 1) { const int32_t t = __shfl_up(s, o, 64); if (lane >= o) s += t; }
        total = __shfl(s, 63, 64);
        return s - v;
    }
    __device__ __forceinline__ int32_t bcast(int32_t v) { return __shfl(v, 0, 64); }
    __device__ __forceinline__ void store16(int32_t off, const uint32_t *w)
    {
        *reinterpret_cast<uint4 *>(dst + off) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __device__ __forceinline__ void bsize(uint32_t v)                       // behind the 16-byte store that wrote zeros there
    {
        __threadfence();
        if (lane == 0) { dst[16] = (uint8_t) v; dst[17] = (uint8_t) (v >> 8); }
    }
    __device__ __forceinline__ uint32_t crc(int32_t len) const
    {
        uint32_t x = crc_slice(GlobalReader{src32}, mis, mis + len, lane, 64);
        for (int o = 32; o > 0; o >>= 1) x ^= (uint32_t) __shfl_xor((int) x, o, 64);
        return crc_join(0xffffffffu, x, mis, mis + len) ^ 0xffffffffu;
    }
};

__global__ __launch_bounds__(64) void k_bgzf_deflate(const uint8_t *__restrict__ data, const int64_t *__restrict__ beg,
                                                     const int32_t *__restrict__ len, int64_t n_blocks, uint8_t *__restrict__ slots,
                                                     int32_t *__restrict__ size)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[kStage / 4];
    __shared__ uint32_t s_hash[kHash], s_freq[kSyms], s_wt[576], s_blc[32], s_misc[mCount];
    __shared__ uint16_t s_tok[kCut], s_mlen[kStep], s_mdist[kStep], s_mhash[kStep], s_code[kSyms], s_cls[320], s_srt[288], s_par[576];
    __shared__ uint8_t s_lens[kSyms];
    const int64_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const Work w{s_hash, s_tok, s_stage, s_mlen, s_mdist, s_mhash, s_freq, s_lens, s_code, s_cls, s_srt, s_wt, s_par, s_blc, s_misc};
    const int64_t at = beg[b];
    WaveDef m;
    m.src = data + at;
    m.src32 = reinterpret_cast<const uint32_t *>(data + (at & ~(int64_t) 3));
    m.mis = (int32_t) (at & 3);
    m.dst = slots + b * dn::kDeflateSlot;
    m.lane = (int) threadIdx.x;
    const int32_t total = deflate_block(m, w, len[b]);
    if (threadIdx.x == 0) size[b] = total;
}

// slot b's size[b] bytes -> out[off[b] ..): 16-byte stores aligned to the destination, their bytes from five aligned
// dwords of the slot (the reads behind a block's last byte stay inside its slot); single bytes before and behind them
__global__ __launch_bounds__(256) void k_deflate_compact(const uint8_t *__restrict__ slots, const int32_t *__restrict__ size,
                                                         const int64_t *__restrict__ off, int64_t n_blocks, uint8_t *__restrict__ out)
{
    const int64_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const uint8_t *s = slots + b * dn::kDeflateSlot;
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(s);
    const int64_t d = off[b];
    const int32_t n = size[b], tid = (int32_t) threadIdx.x;
    int32_t head = (int32_t) ((16 - (d & 15)) & 15);
    if (head > n) head = n;
    if (tid < head) out[d + tid] = s[tid];
    const int32_t n_vec = (n - head) >> 4;
    for (int32_t v = tid; v < n_vec; v += 256) {
        const int32_t sp = head + 16 * v;
        const uint32_t sh = 8u * (uint32_t) (sp & 3);
        uint32_t x[5];
        for (int k = 0; k < 5; k++) x[k] = s32[(sp >> 2) + k];
        uint4 q;
        q.x = (uint32_t) ((((uint64_t) x[1] << 32) | x[0]) >> sh);
        q.y = (uint32_t) ((((uint64_t) x[2] << 32) | x[1]) >> sh);
        q.z = (uint32_t) ((((uint64_t) x[3] << 32) | x[2]) >> sh);
        q.w = (uint32_t) ((((uint64_t) x[4] << 32) | x[3]) >> sh);
        *reinterpret_cast<uint4 *>(out + d + sp) = q;
    }
    const int32_t tail = head + 16 * n_vec;
    if (tail + tid < n) out[d + tail + tid] = s[tail + tid];
}

int bad(const std::string &msg) { return dn::fail(DN_E_INVALID, msg); }

}  // namespace

int64_t dn::deflate_bound(int64_t len)
{
    if (len < 0 || len > kDeflateMaxLen) return -1;
    const int64_t blocks = len == 0 ? 1 : (len + kCut - 1) / kCut;
    return len + 26 + 6 * blocks;
}

int dn::deflate_validate(const char *who, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, const uint8_t *out,
                         int64_t out_cap, const int64_t *out_off)
{
    const std::string w(who);
    if (n_data < 0 || n_blocks < 0 || out_cap < 0 || !out_off || (n_blocks > 0 && (!beg || !len || !out))) return bad(w + ": bad argument");
    int64_t need = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
        if (len[b] < 0 || len[b] > kDeflateMaxLen) return bad(w + ": block " + std::to_string(b) + " has a length outside 0 .. 65280");
        if (beg[b] < 0 || beg[b] > n_data || len[b] > n_data - beg[b]) return bad(w + ": block " + std::to_string(b) + " lies outside the data");
        need += deflate_bound(len[b]);
    }
    if (out_cap < need) return bad(w + ": out_cap is " + std::to_string(out_cap) + ", the blocks may need " + std::to_string(need) + " bytes");
    return DN_OK;
}

int dn::deflate_host(const uint8_t *data, int64_t /*n_data*/, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *out, int64_t *out_off)
{
    std::vector<HostWork> hw(1);
    std::vector<uint8_t> slot((size_t) kDeflateSlot);
    const Work w = hw[0].work();
    out_off[0] = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
        HostDef m{data + beg[b], slot.data()};
        const int32_t total = deflate_block(m, w, len[b]);
        memcpy(out + out_off[b], slot.data(), (size_t) total);
        out_off[b + 1] = out_off[b] + total;
    }
    return DN_OK;
}

int dn::deflate_device(hipStream_t st, const uint8_t *d_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *region,
                       int64_t region_bytes, DeflateTables &t, uint8_t *out, int64_t *out_off, double *ms)
{
    out_off[0] = 0;
    if (n_blocks == 0) return DN_OK;
    const int64_t batch = std::min<int64_t>(std::min<int64_t>(n_blocks, region_bytes / kDeflateRegionPerBlock), 1 << 20);
    if (batch < 1) return dn::fail(DN_E_INVALID, "deflate_device: the region holds no block");
    uint8_t *compact = region + batch * kDeflateSlot;
    if (!t.e0) { DN_TRY(t.e0.create(hipEventCreate)); DN_TRY(t.e1.create(hipEventCreate)); }
    DN_TRY(t.beg.reserve(batch, 0, st)); DN_TRY(t.off.reserve(batch, 0, st));
    DN_TRY(t.len.reserve(batch, 0, st)); DN_TRY(t.size.reserve(batch, 0, st));
    t.h_size.resize((size_t) batch);
    t.h_off.resize((size_t) batch);
    for (int64_t first = 0; first < n_blocks; first += batch) {
        const int64_t nb = std::min(batch, n_blocks - first);
        float a = 0.f, c = 0.f;
        DN_TRY(hipMemcpyAsync(t.beg, beg + first, sizeof(int64_t) * (size_t) nb, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(t.len, len + first, sizeof(int32_t) * (size_t) nb, hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(t.e0, st));
        hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned) nb), dim3(64), 0, st, d_data, (const int64_t *) t.beg.get(), (const int32_t *) t.len.get(), nb,
                           region, t.size.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(t.e1, st));
        DN_TRY(hipMemcpyAsync(t.h_size.data(), t.size, sizeof(int32_t) * (size_t) nb, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        DN_TRY(hipEventElapsedTime(&a, t.e0, t.e1));
        int64_t total = 0;
        for (int64_t k = 0; k < nb; k++) {
            if (t.h_size[(size_t) k] < 28 || t.h_size[(size_t) k] > deflate_bound(len[first + k]))
                return dn::fail(DN_E_STATE, "deflate_device: block " + std::to_string(first + k) + " came back with the size " + std::to_string(t.h_size[(size_t) k]));
            t.h_off[(size_t) k] = total;
            total += t.h_size[(size_t) k];
        }
        DN_TRY(hipMemcpyAsync(t.off, t.h_off.data(), sizeof(int64_t) * (size_t) nb, hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(t.e0, st));
        hipLaunchKernelGGL(k_deflate_compact, dim3((unsigned) nb), dim3(256), 0, st, (const uint8_t *) region, (const int32_t *) t.size.get(),
                           (const int64_t *) t.off.get(), nb, compact);
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(t.e1, st));
        DN_TRY(hipMemcpyAsync(out + out_off[first], compact, (size_t) total, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        DN_TRY(hipEventElapsedTime(&c, t.e0, t.e1));
        if (ms) *ms += (double) a + (double) c;
        for (int64_t k = 0; k < nb; k++) out_off[first + k + 1] = out_off[first] + t.h_off[(size_t) k] + t.h_size[(size_t) k];
    }
    return DN_OK;
}

extern "C" int64_t dn_bgzf_deflate_bound(int64_t n_blocks, const int32_t *len)
{
    int64_t sum = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
        const int64_t one = len ? dn::deflate_bound(len[b]) : -1;
        if (one < 0) return -1;
        sum += one;
    }
    return n_blocks < 0 ? -1 : sum;
}

extern "C" int dn_bgzf_deflate_host(const uint8_t *data, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *out,
                                    int64_t out_cap, int64_t *out_off)
{
    dn::clear_error();
    const int rc = dn::deflate_validate("dn_bgzf_deflate_host", n_data, n_blocks, beg, len, out, out_cap, out_off);
    if (rc != DN_OK) return rc;
    if (n_data > 0 && !data) return bad("dn_bgzf_deflate_host: bad argument");
    return dn::deflate_host(data, n_data, n_blocks, beg, len, out, out_off);
}

extern "C" int dn_bgzf_deflate(int device, const uint8_t *data, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len,
                               uint8_t *out, int64_t out_cap, int64_t *out_off, double *device_ms)
{
    dn::clear_error();
    const int rc = dn::deflate_validate("dn_bgzf_deflate", n_data, n_blocks, beg, len, out, out_cap, out_off);
    if (rc != DN_OK) return rc;
    if (device < 0 || (n_data > 0 && !data)) return bad("dn_bgzf_deflate: bad argument");
    if (device_ms) *device_ms = 0.0;
    out_off[0] = 0;
    if (n_blocks == 0) return DN_OK;
    constexpr int64_t kBatch = 1024;                    // blocks in flight: 128 MiB of slots and compacted output
    const int64_t region_bytes = std::min(n_blocks, kBatch) * dn::kDeflateRegionPerBlock;
    dn::Stream st;
    dn::DeviceBuffer<uint8_t> d_data, region;
    dn::DeflateTables t;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(d_data.alloc((size_t) n_data + 64));
        DN_TRY(region.alloc((size_t) region_bytes));
        if (n_data > 0) DN_TRY(hipMemcpyAsync(d_data, data, (size_t) n_data, hipMemcpyHostToDevice, st));
        return dn::deflate_device(st, d_data, n_blocks, beg, len, region, region_bytes, t, out, out_off, device_ms);
    });
}

extern "C" int dn_deflate_code_lengths_host(const uint32_t *freq, int32_t n, int32_t limit, uint8_t *lens)
{
    dn::clear_error();
    if (!freq || !lens || n < 1 || n > 288 || limit < 1 || limit > 15 || (1 << limit) < n)
        return bad("dn_deflate_code_lengths_host: bad argument (n is 1 .. 288, limit 1 .. 15 and 2^limit at least n)");
    std::vector<HostWork> hw(1);
    HostDef m{nullptr, nullptr};
    build_lengths(m, hw[0].work(), freq, n, limit, lens);
    return DN_OK;
}

// dn_text.hpp -- one float64 -> its '%.5f' text, and one line of a coverage file (include/degnorm_amd.h, "Coverage
// matrices to text", defines the rule).  One source for both builds: put_value and walk_line are __host__ __device__ code,
//   E   whether the text is written.  walk_line<false> walks a line's values and returns its width; walk_line<true>
//       walks them again and writes the bytes.  The walk is the same in both, so what the second writes is what the first
//       measured, and no store goes outside the window it was given (Window).
// The device build writes a line through windows of the wavefront's LDS chunk, the host build through one window that is
// the line itself; a value that straddles a window's end is formatted again in the next window, clipped on the other side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef DN_HD
#define DN_HD __host__ __device__ __forceinline__
#endif

namespace dn {
namespace text {

// Stores of the text bytes [lo, hi) -- offsets in the batch's text -- at p, where p[0] is the byte at offset `base`;
// E = false: none.
template <bool E> struct Window {
    uint8_t *p;
    int64_t base, lo, hi;
    DN_HD void put(int64_t o, uint32_t c) const
    {
        if (E && o >= lo && o < hi) p[o - base] = (uint8_t) c;
    }
};

constexpr uint32_t kE9 = 1000000000u;
constexpr int kMaxValue = 1 + 19 + 6;                 // '-', the digits of 2^63 - 1, '.' and five digits

DN_HD int digits32(uint32_t v)
{
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7
           : v < 100000000u ? 8 : v < kE9 ? 9 : 10;
}

// the nd low decimal digits of v at [at, at + nd), leading zeros included
template <bool E> DN_HD void put_digits(const Window<E> &w, int64_t at, uint32_t v, int nd)
{
    if (!E) return;
    for (int k = nd - 1; k >= 0; k--) {
        w.put(at + k, '0' + v % 10u);
        v /= 10u;
    }
}

// |x| 10^5 rounded half to even, as integer part I and q < 10^5 (I 10^5 + q is the rounded number: 10^5 is even, so q
// alone decides a tie).  false: NaN, an infinity or |x| >= 2^63.
DN_HD bool scaled(uint64_t bits, uint64_t *I, uint32_t *q)
{
    const int ex = (int) ((bits >> 52) & 0x7ffu);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    if (ex >= 1023 + 63) return false;                  // also NaN and the infinities (ex = 2047)
    const uint64_t m = ex ? frac | (1ull << 52) : frac; // |x| = m 2^e
    const int e = ex ? ex - 1075 : -1074;
    if (e >= 0) {                                       // e <= 10: an integer below 2^63
        *I = m << e;
        *q = 0;
        return true;
    }
    const int s = -e;                                   // 1 .. 1074 fraction bits
    const uint64_t f = s < 64 ? m & ((1ull << s) - 1) : m;
    *I = s < 64 ? m >> s : 0;
    // f 3125 in two words: f = a 2^32 + b with a < 2^21
    const uint64_t pa = (f >> 32) * 3125u, pb = (f & 0xffffffffu) * 3125u;
    const uint64_t lo = (pa << 32) + pb;
    const uint64_t hi = (pa >> 32) + (lo < pb ? 1u : 0u);
    const int r = s - 5;                                // the fraction times 10^5 is (hi, lo) / 2^r
    uint64_t v;
    if (r <= 0) {
        v = lo << -r;                                   // s < 5: f < 16, exact
    } else if (r >= 66) {
        v = 0;                                          // (hi, lo) < 2^65 <= half
    } else {
        const int h = r - 1;                            // the bit that is one half
        v = r < 64 ? (lo >> r) | (hi << (64 - r)) : hi >> (r - 64);         // r < 64 here has r >= 1; hi < 2
        const uint64_t half = h < 64 ? (lo >> h) & 1u : (hi >> (h - 64)) & 1u;
        const bool below = h == 0 ? false : h < 64 ? (lo & ((1ull << h) - 1)) != 0 : lo != 0;   // bits below one half
        if (half && (below || (v & 1u))) v++;
    }
    if (v >= 100000u) {                                 // the fraction rounded up to one
        v -= 100000u;
        *I += 1;
    }
    *q = (uint32_t) v;
    return true;
}

// the text of one value at offset `at`: its width, or 0 for a value the rule does not cover
template <bool E> DN_HD int put_value(uint64_t bits, const Window<E> &w, int64_t at)
{
    uint64_t I;
    uint32_t q;
    if (!scaled(bits, &I, &q)) return 0;
    const int sign = (int) (bits >> 63);
    if (sign) w.put(at, '-');
    at += sign;
    int nd;
    if (I < kE9) {
        nd = digits32((uint32_t) I);
        put_digits(w, at, (uint32_t) I, nd);
    } else {
        const uint64_t up = I / kE9;                    // below 2^63 / 10^9 < 10^10
        const uint32_t low = (uint32_t) (I % kE9);
        if (up < kE9) {
            nd = digits32((uint32_t) up);
            put_digits(w, at, (uint32_t) up, nd);
        } else {
            nd = 10;
            w.put(at, '0' + (uint32_t) (up / kE9));
            put_digits(w, at + 1, (uint32_t) (up % kE9), 9);
        }
        put_digits(w, at + nd, low, 9);
        nd += 9;
    }
    w.put(at + nd, '.');
    put_digits(w, at + nd + 1, q, 5);
    return sign + nd + 6;
}

DN_HD uint64_t bits_of(double x)
{
    union { double d; uint64_t u; } c;
    c.d = x;
    return c.u;
}

// One line: the values x[i * stride], i < p, each followed by ' ' or, the last one, by '\n'.  The walk goes on from value
// *i, whose text begins at *at, while values begin below w.hi; it stops in front of a value that reaches beyond w.hi after
// writing the part inside, so that the next window takes it up again.  *bad is set by a value the rule does not cover,
// which counts as no bytes.  With w.hi above every offset this is the whole line and *at ends one behind it.
template <bool E> DN_HD void walk_line(const double *x, int64_t stride, int p, int *i, int64_t *at, const Window<E> &w, bool *bad)
{
    while (*i < p && *at < w.hi) {
        const int n = put_value<E>(bits_of(x[(int64_t) *i * stride]), w, *at);
        if (n == 0) *bad = true;
        w.put(*at + n, *i + 1 < p ? ' ' : '\n');
        if (*at + n + 1 > w.hi) return;
        *at += n + 1;
        *i += 1;
    }
}

}  // namespace text
}  // namespace dn

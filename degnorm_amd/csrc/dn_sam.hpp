// dn_sam.hpp -- one SAM alignment line -> one BAM record (include/degnorm_amd.h, "SAM text to BAM records", defines the
// encoding).  One source for both builds: encode_line is __host__ __device__ code against two policies,
//   M   where the text is read (dn_fields.hpp, which also has the hash, the digits and the word test used here): Bytes on
//       the device, HostText on the host.
//   E   whether the record is written.  encode_line<M, false> walks the line, checks every field and returns
//       the record's size and its number of float payloads; encode_line<M, true> walks it again and writes every byte of
//       the record except the float payloads, for which it notes (place in the record stream, place in the text).
// The walk is the same in both, field after field, so the first error of a line is the same whoever finds it, and what
// the second walk writes is what the first one measured.  No store goes beyond the size the first walk returned (Writer).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/degnorm_amd.h"
#include "dn_bam_record.hpp"
#include "dn_fields.hpp"

namespace dn {
namespace sam {

// The @SQ names in ascending order of the FNV-1a hash of the name: entry k is reference id[k], whose name is the
// name_len[k] bytes at names + name_beg[k].
struct Refs {
    int32_t n;
    const uint64_t *hash;
    const int32_t *id;
    const int64_t *name_beg;
    const int32_t *name_len;
    const uint8_t *names;
};

// what a line becomes: the bytes of its record, block_size word included, and its float payloads
struct LineSize {
    int64_t size, n_float;
};

// Stores of the record at p, which has `cap` bytes; E = false: none.  Byte stores: fields lie at any offset.
template <bool E> struct Writer {
    uint8_t *p;
    int64_t cap;
    DN_HD void u8(int64_t o, uint32_t v) const
    {
        if (E && o >= 0 && o < cap) p[o] = (uint8_t) v;
    }
    DN_HD void u16(int64_t o, uint32_t v) const { u8(o, v & 0xffu); u8(o + 1, (v >> 8) & 0xffu); }
    DN_HD void u32(int64_t o, uint32_t v) const { u16(o, v & 0xffffu); u16(o + 2, v >> 16); }
};

constexpr int64_t kMaxCigarLen = (1 << 28) - 1;         // an op is len << 4 | code in 32 bits
constexpr int kMaxCigarOps = 65535;
constexpr int kMaxName = 254;

// the end of the field that starts at a: the next tab, or end
template <class M> DN_HD int64_t field_end(M &in, int64_t a, int64_t end)
{
    while (a < end && in.at(a) != '\t') a++;
    return a;
}

// [lo, hi) as a decimal integer: an optional '-' (sign) or '+' (plus), then 1 .. 18 digits and nothing else
template <class M> DN_HD bool parse_int(M &in, int64_t lo, int64_t hi, bool sign, bool plus, int64_t *out)
{
    bool neg = false;
    if (lo < hi) {
        const uint32_t c = in.at(lo);
        if ((c == '-' && sign) || (c == '+' && plus)) { neg = c == '-'; lo++; }
    }
    int64_t v = 0;
    if (!parse_uint(in, lo, hi, &v)) return false;
    *out = neg ? -v : v;
    return true;
}

template <class M> DN_HD bool parse_range(M &in, int64_t lo, int64_t hi, bool sign, int64_t vmin, int64_t vmax, int64_t *out)
{
    return parse_int(in, lo, hi, sign, false, out) && *out >= vmin && *out <= vmax;
}

// [lo, hi) is text strtod reads whole as a decimal number: [+-] then inf, infinity, nan, or digits with at most one '.'
// and at least one digit, then optionally e or E, [+-] and digits.  The value is not computed here.
template <class M> DN_HD bool float_syntax(M &in, int64_t lo, int64_t hi)
{
    int64_t p = lo;
    if (p < hi && (in.at(p) == '+' || in.at(p) == '-')) p++;
    if (spells(in, p, hi, "inf", 3) || spells(in, p, hi, "infinity", 8) || spells(in, p, hi, "nan", 3)) return true;
    int nd = 0;
    while (p < hi && in.at(p) >= '0' && in.at(p) <= '9') { p++; nd++; }
    if (p < hi && in.at(p) == '.') {
        p++;
        while (p < hi && in.at(p) >= '0' && in.at(p) <= '9') { p++; nd++; }
    }
    if (nd == 0) return false;
    if (p < hi && (in.at(p) | 0x20u) == 'e') {
        p++;
        if (p < hi && (in.at(p) == '+' || in.at(p) == '-')) p++;
        int ne = 0;
        while (p < hi && in.at(p) >= '0' && in.at(p) <= '9') { p++; ne++; }
        if (ne == 0) return false;
    }
    return p == hi;
}

// refID of the name [lo, hi), -2 when the table does not have it
template <class M> DN_HD int32_t find_ref(M &in, int64_t lo, int64_t hi, const Refs &R)
{
    const uint64_t h = fnv1a(in, lo, hi);
    int32_t a = 0, b = R.n;                         // the first entry whose hash is not below h
    while (a < b) {
        const int32_t mid = a + ((b - a) >> 1);
        if (R.hash[mid] < h) a = mid + 1; else b = mid;
    }
    for (; a < R.n && R.hash[a] == h; a++) {
        if ((int64_t) R.name_len[a] != hi - lo) continue;
        const uint8_t *nm = R.names + R.name_beg[a];
        bool same = true;
        for (int64_t k = 0; k < hi - lo && same; k++) same = in.at(lo + k) == (uint32_t) nm[k];
        if (same) return R.id[a];
    }
    return -2;
}

DN_HD uint32_t base_code(uint32_t c)
{
    switch (c | 0x20u) {
    case 'a': return 1; case 'c': return 2; case 'm': return 3; case 'g': return 4; case 'r': return 5; case 's': return 6;
    case 'v': return 7; case 't': return 8; case 'w': return 9; case 'y': return 10; case 'h': return 11; case 'k': return 12;
    case 'd': return 13; case 'b': return 14;
    default: return c == '=' ? 0u : 15u;
    }
}

// the code of a CIGAR operation letter in MIDNSHP=X, -1 for another byte
DN_HD int cigar_code(uint32_t c)
{
    switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
    default: return -1;
    }
}

// bytes of a value of B subtype t, 0 for a byte that is none; the range of an integer subtype
DN_HD int array_width(uint32_t t)
{
    return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' || t == 'f' ? 4 : 0;
}
DN_HD bool array_fits(uint32_t t, int64_t v)
{
    switch (t) {
    case 'c': return v >= -128 && v <= 127;
    case 'C': return v >= 0 && v <= 255;
    case 's': return v >= -32768 && v <= 32767;
    case 'S': return v >= 0 && v <= 65535;
    case 'i': return v >= -2147483648ll && v <= 2147483647ll;
    default: return v >= 0 && v <= 4294967295ll;       // 'I'
    }
}

// One optional field [a, z) -> its bytes from record offset o on; *o moves behind them.  Float payloads are left out:
// payload number *nf of the line is noted as patch[2 * nf] = rec_abs + its record offset, patch[2 * nf + 1] = where its text
// starts (patch may be null when E is false).  0 or a DN_SAM_E_*.
template <class M, bool E>
DN_HD int encode_field(M &in, int64_t a, int64_t z, const Writer<E> &w, int64_t *o, int64_t rec_abs, int64_t *patch, int64_t patch_cap,
                       int64_t *nf)
{
    if (z - a < 5 || in.at(a + 2) != ':' || in.at(a + 4) != ':') return DN_SAM_E_TAG;
    const uint32_t type = in.at(a + 3);
    const int64_t v = a + 5;
    int64_t q = *o;
    w.u8(q, in.at(a)); w.u8(q + 1, in.at(a + 1));
    q += 2;
    const auto note_float = [&](int64_t at, int64_t text) {
        if (E && patch && *nf < patch_cap) { patch[2 * *nf] = rec_abs + at; patch[2 * *nf + 1] = text; }
        w.u32(at, 0);
        ++*nf;
    };
    if (type == 'A') {
        if (z - v != 1) return DN_SAM_E_TAG;
        w.u8(q, 'A'); w.u8(q + 1, in.at(v));
        q += 2;
    } else if (type == 'i') {
        int64_t x = 0;
        if (!parse_int(in, v, z, true, true, &x)) return DN_SAM_E_TAG;
        if (x < -2147483648ll || x > 4294967295ll) return DN_SAM_E_TAG_RANGE;
        const bool neg = x < 0;
        const int width = neg ? (x >= -128 ? 1 : x >= -32768 ? 2 : 4) : (x <= 255 ? 1 : x <= 65535 ? 2 : 4);
        w.u8(q, width == 1 ? (neg ? 'c' : 'C') : width == 2 ? (neg ? 's' : 'S') : (neg ? 'i' : 'I'));
        const uint32_t bits = (uint32_t) (uint64_t) x;
        if (width == 1) w.u8(q + 1, bits & 0xffu); else if (width == 2) w.u16(q + 1, bits & 0xffffu); else w.u32(q + 1, bits);
        q += 1 + width;
    } else if (type == 'f') {
        if (!float_syntax(in, v, z)) return DN_SAM_E_TAG_FLOAT;
        w.u8(q, 'f');
        note_float(q + 1, v);
        q += 5;
    } else if (type == 'Z' || type == 'H') {
        if (type == 'H' && ((z - v) & 1)) return DN_SAM_E_TAG_HEX;
        w.u8(q, type);
        for (int64_t p = v; p < z; p++) w.u8(q + 1 + (p - v), in.at(p));
        w.u8(q + 1 + (z - v), 0);
        q += 2 + (z - v);
    } else if (type == 'B') {
        const uint32_t t = v < z ? in.at(v) : 0;
        const int width = array_width(t);
        if (width == 0) return DN_SAM_E_TAG;
        w.u8(q, 'B'); w.u8(q + 1, t);
        int64_t count = 0, p = v + 1, at = q + 6;
        while (p < z) {
            if (in.at(p) != ',') return DN_SAM_E_TAG;
            int64_t e = p + 1;
            while (e < z && in.at(e) != ',') e++;
            if (t == 'f') {
                if (!float_syntax(in, p + 1, e)) return DN_SAM_E_TAG_FLOAT;
                note_float(at, p + 1);
            } else {
                int64_t x = 0;
                if (!parse_int(in, p + 1, e, true, true, &x)) return DN_SAM_E_TAG;
                if (!array_fits(t, x)) return DN_SAM_E_TAG_ARRAY;
                const uint32_t bits = (uint32_t) (uint64_t) x;
                if (width == 1) w.u8(at, bits & 0xffu); else if (width == 2) w.u16(at, bits & 0xffffu); else w.u32(at, bits);
            }
            at += width;
            count++;
            p = e;
        }
        w.u32(q + 2, (uint32_t) count);
        q = at;
    } else {
        return DN_SAM_E_TAG;
    }
    *o = q;
    return 0;
}

// The line [beg, end) of the text (without its '\n') -> L, and with E its record at rec (L.size bytes as measured before,
// passed in as cap; the record starts at byte rec_abs of the stream) and the line's entries of the patch table.
// 0 or the DN_SAM_E_* of the first fault of the line.
template <class M, bool E>
DN_HD int encode_line(M &in, int64_t beg, int64_t end, const Refs &R, uint8_t *rec, int64_t cap, int64_t rec_abs, int64_t *patch,
                      int64_t patch_cap, LineSize &L)
{
    const Writer<E> w{rec, cap};
    L.size = 0; L.n_float = 0;
    if (end > beg && in.at(end - 1) == '\r') end--;
    if (end <= beg) return DN_SAM_E_EMPTY;
    int64_t a = beg, z = 0, x = 0;
#define DN_SAM_NEXT()                               \
    if (z >= end) return DN_SAM_E_FIELDS;           \
    a = z + 1;                                      \
    z = field_end(in, a, end);
    // QNAME
    z = field_end(in, a, end);
    if (z >= end) return DN_SAM_E_FIELDS;
    const int64_t l_name = z - a + 1;                 // with its NUL
    if (l_name < 2 || l_name > kMaxName + 1) return DN_SAM_E_NAME;
    for (int64_t p = a; p < z; p++) w.u8(kBamName + (p - a), in.at(p));
    w.u8(kBamName + l_name - 1, 0);
    // FLAG
    DN_SAM_NEXT();
    if (!parse_range(in, a, z, false, 0, 65535, &x)) return DN_SAM_E_INTEGER;
    const uint32_t flag = (uint32_t) x;
    // RNAME
    DN_SAM_NEXT();
    const int32_t ref = z - a == 1 && in.at(a) == '*' ? -1 : find_ref(in, a, z, R);
    if (ref < -1) return DN_SAM_E_RNAME;
    // POS
    DN_SAM_NEXT();
    if (!parse_range(in, a, z, false, 0, 2147483647ll, &x)) return DN_SAM_E_INTEGER;
    const int64_t pos = x - 1;
    // MAPQ
    DN_SAM_NEXT();
    if (!parse_range(in, a, z, false, 0, 255, &x)) return DN_SAM_E_INTEGER;
    const uint32_t mapq = (uint32_t) x;
    // CIGAR
    DN_SAM_NEXT();
    int64_t n_ops = 0, qlen = 0, rlen = 0;
    if (!(z - a == 1 && in.at(a) == '*')) {
        if (z == a) return DN_SAM_E_CIGAR;
        int64_t len = 0;
        int nd = 0;
        for (int64_t p = a; p < z; p++) {
            const uint32_t c = in.at(p);
            if (c >= '0' && c <= '9') {
                len = len * 10 + (int64_t) (c - '0');
                nd++;
                if (len > kMaxCigarLen) return DN_SAM_E_CIGAR;
                continue;
            }
            const int code = cigar_code(c);
            if (code < 0 || nd == 0) return DN_SAM_E_CIGAR;
            if (n_ops == kMaxCigarOps) return DN_SAM_E_CIGAR_OPS;
            w.u32(kBamName + l_name + 4 * n_ops, (uint32_t) len << 4 | (uint32_t) code);
            if (code == 0 || code == 1 || code == 4 || code == 7 || code == 8) qlen += len;
            if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) rlen += len;
            n_ops++;
            len = 0;
            nd = 0;
        }
        if (nd != 0) return DN_SAM_E_CIGAR;
    }
    // RNEXT
    DN_SAM_NEXT();
    int32_t next_ref = -1;
    if (z - a == 1 && in.at(a) == '=') next_ref = ref;
    else if (!(z - a == 1 && in.at(a) == '*')) next_ref = find_ref(in, a, z, R);
    if (next_ref < -1) return DN_SAM_E_RNAME;
    // PNEXT, TLEN
    DN_SAM_NEXT();
    if (!parse_range(in, a, z, false, 0, 2147483647ll, &x)) return DN_SAM_E_INTEGER;
    const int64_t next_pos = x - 1;
    DN_SAM_NEXT();
    if (!parse_range(in, a, z, true, -2147483648ll, 2147483647ll, &x)) return DN_SAM_E_INTEGER;
    const int64_t tlen = x;
    // SEQ
    DN_SAM_NEXT();
    if (z == a) return DN_SAM_E_SEQ;
    const bool no_seq = z - a == 1 && in.at(a) == '*';
    const int64_t l_seq = no_seq ? 0 : z - a;
    if (!no_seq && n_ops > 0 && qlen != l_seq) return DN_SAM_E_SEQ_CIGAR;
    const int64_t seq_at = kBamName + l_name + 4 * n_ops, qual_at = seq_at + (l_seq + 1) / 2;
    for (int64_t k = 0; k < l_seq; k += 2) {
        const uint32_t hi = base_code(in.at(a + k)), lo = k + 1 < l_seq ? base_code(in.at(a + k + 1)) : 0u;
        w.u8(seq_at + (k >> 1), hi << 4 | lo);
    }
    // QUAL
    DN_SAM_NEXT();
    if (z - a == 1 && in.at(a) == '*') {
        for (int64_t k = 0; k < l_seq; k++) w.u8(qual_at + k, 0xffu);
    } else {
        if (z == a || z - a != l_seq) return DN_SAM_E_QUAL_LEN;
        for (int64_t k = 0; k < l_seq; k++) {
            const uint32_t c = in.at(a + k);
            if (c < 33 || c > 126) return DN_SAM_E_QUAL;
            w.u8(qual_at + k, c - 33);
        }
    }
    // optional fields
    int64_t o = qual_at + l_seq, nf = 0;
    while (z < end) {
        a = z + 1;
        z = field_end(in, a, end);
        const int e = encode_field<M, E>(in, a, z, w, &o, rec_abs, patch, patch_cap, &nf);
        if (e) return e;
    }
#undef DN_SAM_NEXT
    const int64_t end_pos = pos + (rlen > 1 ? rlen : 1);
    w.u32(0, (uint32_t) (o - 4));
    w.u32(kBamRef, (uint32_t) ref);
    w.u32(kBamPos, (uint32_t) (int32_t) pos);
    w.u8(kBamLName, (uint32_t) l_name);
    w.u8(kBamLName + 1, mapq);
    w.u16(kBamLName + 2, reg2bin(pos, end_pos) & 0xffffu);
    w.u16(kBamNCigar, (uint32_t) n_ops);
    w.u16(kBamFlag, flag);
    w.u32(kBamLSeq, (uint32_t) l_seq);
    w.u32(kBamNextRef, (uint32_t) next_ref);
    w.u32(kBamNextPos, (uint32_t) (int32_t) next_pos);
    w.u32(kBamNextPos + 4, (uint32_t) (int32_t) tlen);
    L.size = o;
    L.n_float = nf;
    return 0;
}

}  // namespace sam
}  // namespace dn

// dn_fields.hpp -- what a tab-separated text line is made of, for the rules of the three text readers (dn_gtf.hpp,
// dn_gff3.hpp, dn_sam.hpp): a hash of a span, an unsigned integer, a word in any letter case, the nine fields of an
// annotation line and its `exon` test.  All are __host__ __device__ templates over a byte reader M, where at(pos) gives the
// byte at pos.  The device build reads aligned 8-byte words of a buffer padded to whole tiles (Bytes, dn_lines.hpp); the host
// build reads the caller's bytes as they are (HostText), so a read past a line's end is a read past the buffer for the last
// line and a sanitizer sees it.  No function here reads outside the span it is given.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// dn_sam.hpp includes dn_bam_record.hpp first and so keeps that header's DN_HD for the code here
#ifndef DN_HD
#define DN_HD __host__ __device__ inline
#endif

namespace dn {

struct HostText {
    const uint8_t *p;
    DN_HD uint32_t at(int64_t pos) const { return p[pos]; }
};

// what a line of an annotation becomes: nothing, or an exon row (dn_gff3.hpp adds two more kinds)
enum { kSkip = 0, kExon = 1 };

// FNV-1a, 64 bits
template <class M> DN_HD uint64_t fnv1a(M &in, int64_t lo, int64_t hi)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t p = lo; p < hi; p++) h = (h ^ in.at(p)) * 0x100000001b3ull;
    return h;
}

// [lo, hi) as a decimal integer of 1 .. 18 digits and nothing else
template <class M> DN_HD bool parse_uint(M &in, int64_t lo, int64_t hi, int64_t *out)
{
    if (hi <= lo || hi - lo > 18) return false;
    int64_t v = 0;
    for (int64_t p = lo; p < hi; p++) {
        const uint32_t c = in.at(p);
        if (c < '0' || c > '9') return false;
        v = v * 10 + (int64_t) (c - '0');
    }
    *out = v;
    return true;
}

// does [lo, hi) spell `word` (n lower-case letters) in any letter case?
template <class M> DN_HD bool spells(M &in, int64_t lo, int64_t hi, const char *word, int n)
{
    if (hi - lo != n) return false;
    for (int k = 0; k < n; k++)
        if ((in.at(lo + k) | 0x20u) != (uint32_t) word[k]) return false;
    return true;
}

// the tabs that end fields 1 to 5 and field 8 of an annotation line; field nine starts behind t8
struct NineFields {
    int64_t t1, t2, t3, t4, t5, t8;
};

// the walk over the first eight tabs of the line [beg, end); false: fewer than nine fields
template <class M> DN_HD bool nine_fields(M &in, int64_t beg, int64_t end, NineFields &F)
{
    F = NineFields{0, 0, 0, 0, 0, 0};
    int nt = 0;
    for (int64_t p = beg; p < end; p++) {
        if (in.at(p) != '\t') continue;
        nt++;
        if (nt == 1) F.t1 = p;
        else if (nt == 2) F.t2 = p;
        else if (nt == 3) F.t3 = p;
        else if (nt == 4) F.t4 = p;
        else if (nt == 5) F.t5 = p;
        else if (nt == 8) { F.t8 = p; break; }
    }
    return nt == 8;
}

// Field seven of the annotation line that starts at beg, for the optional strand column of both scans: the byte when the
// field is exactly one of + - . ? and 0 otherwise.  The walk ends at the sixth tab, at a '\n' or at `limit`, whichever comes
// first, so it stays inside the line and below limit.
template <class M> DN_HD uint8_t strand_field(M &in, int64_t beg, int64_t limit)
{
    int nt = 0;
    int64_t p = beg;
    while (p < limit && nt < 6) {
        const uint32_t c = in.at(p++);
        if (c == '\n') return 0;
        if (c == '\t') nt++;
    }
    if (nt < 6 || p + 1 >= limit || in.at(p + 1) != '\t') return 0;
    const uint32_t c = in.at(p);
    return c == '+' || c == '-' || c == '.' || c == '?' ? (uint8_t) c : 0;
}

// is field three `exon` in any letter case?
template <class M> DN_HD bool is_exon(M &in, const NineFields &F) { return spells(in, F.t2 + 1, F.t3, "exon", 4); }

}  // namespace dn

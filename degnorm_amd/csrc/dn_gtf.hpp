// dn_gtf.hpp -- one GTF line -> an exon row (include/degnorm_amd.h, dn_gtf_scan, defines the rule).  As dn_gff3.hpp and
// dn_sam.hpp: __host__ __device__ templates over a byte reader M (dn_fields.hpp).  k_parse_lines (dn_gtf.hip) runs them on
// Bytes; tools/gtf_host_check.hip runs them on HostText from buffers of exactly the text's size under the host sanitizers.
// Every read of parse_line lies in [beg, end) of its line, and every loop ends at the line's end or before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/degnorm_amd.h"
#include "dn_fields.hpp"

namespace dn {
namespace gtf {

// does [p, end) begin with tag (n bytes)?
template <class M> DN_HD bool begins_with(M &in, int64_t p, int64_t end, const char *tag, int n)
{
    if (end - p < n) return false;
    for (int k = 0; k < n; k++)
        if (in.at(p + k) != (uint32_t) tag[k]) return false;
    return true;
}

// [*lo, *hi) without blanks and double quotes at either end
template <class M> DN_HD void strip_value(M &in, int64_t *lo, int64_t *hi)
{
    int64_t a = *lo, z = *hi;
    while (a < z) { const uint32_t c = in.at(a); if (c != ' ' && c != '"') break; a++; }
    while (z > a) { const uint32_t c = in.at(z - 1); if (c != ' ' && c != '"') break; z--; }
    *lo = a; *hi = z;
}

// The gene name of attribute field [a, end): pieces between ';', blanks stripped; the first piece that begins with gene_name
// gives it, and when there is none or its value is empty the first piece that begins with gene_id (loaders.py:102-112).
// The field ends at a tab as well.  False: neither gives a value.
template <class M> DN_HD bool gene_of(M &in, int64_t a, int64_t end, int64_t *g_lo, int64_t *g_hi)
{
    bool seen_name = false, seen_id = false;
    int64_t id_lo = 0, id_hi = 0;
    int64_t p = a;
    while (p < end) {
        while (p < end && in.at(p) == ' ') p++;
        const bool is_name = !seen_name && begins_with(in, p, end, "gene_name", 9);
        const bool is_id = !seen_id && !is_name && begins_with(in, p, end, "gene_id", 7);
        int64_t q = p;
        uint32_t c = 0;
        while (q < end) { c = in.at(q); if (c == ';' || c == '\t') break; q++; }
        if (is_name) {
            int64_t lo = p + 9, hi = q;
            strip_value(in, &lo, &hi);
            if (hi > lo) { *g_lo = lo; *g_hi = hi; return true; }
            seen_name = true;
        } else if (is_id) {
            id_lo = p + 7; id_hi = q;
            strip_value(in, &id_lo, &id_hi);
            seen_id = true;
        }
        if (q >= end || c == '\t' || (seen_name && seen_id)) break;
        p = q + 1;
    }
    if (seen_id && id_hi > id_lo) { *g_lo = id_lo; *g_hi = id_hi; return true; }
    return false;
}

// The line [beg, end) of the text (without its '\n') -> kSkip, kExon (the chromosome name is [beg, *chr_end), the gene name
// [*g_lo, *g_hi)) or -(DN_GTF_E_*).
template <class M>
DN_HD int parse_line(M &in, int64_t beg, int64_t end, int64_t *chr_end, int64_t *start, int64_t *stop, int64_t *g_lo, int64_t *g_hi)
{
    if (end > beg && in.at(end - 1) == '\r') end--;
    if (end <= beg || in.at(beg) == '#') return kSkip;
    NineFields F;
    if (!nine_fields(in, beg, end, F)) return -DN_GTF_E_FIELDS;
    if (!is_exon(in, F)) return kSkip;
    if (!parse_uint(in, F.t3 + 1, F.t4, start) || !parse_uint(in, F.t4 + 1, F.t5, stop)) return -DN_GTF_E_INTEGER;
    if (!gene_of(in, F.t8 + 1, end, g_lo, g_hi)) return -DN_GTF_E_GENE;
    *chr_end = F.t1;
    return kExon;
}

}  // namespace gtf
}  // namespace dn

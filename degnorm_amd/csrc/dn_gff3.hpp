// dn_gff3.hpp -- one GFF3 line -> an exon row or a node row, and the walk from an exon's Parent to its gene
// (include/degnorm_amd.h, "GFF3 annotation scan", defines both).  One source for both builds: parse_line and walk are
// __host__ __device__ templates over a byte reader M (dn_fields.hpp, which also has the field walk and the hash they share
// with the GTF rule): Bytes on the device, HostText on the host.
// Every read of parse_line lies in [beg, end) of its line; every read of walk lies inside a span that parse_line cut out of
// a line.  walk makes at most kMaxLookups lookups, and the scan of a run of equal hashes ends at the run's end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/degnorm_amd.h"
#include "dn_fields.hpp"

namespace dn {
namespace gff3 {

constexpr int kMaxLookups = 8;

enum { kNode = 2, kFasta = 3 };         // besides kSkip and kExon (dn_fields.hpp)

// What a line becomes.  An exon row: c = the chromosome name, start, end, a = its gene name (open 0) or the first element of
// its Parent (open 1).  A node row: c = its ID, a = the name an exon that reaches it gets (open 0: gname, or rname when the
// node has no parent) or the first element of its Parent (open 1).  Spans are [lo, hi) in the reader's positions.
struct Line {
    int64_t c_lo, c_hi, start, end, a_lo, a_hi;
    int open;
};

DN_HD uint64_t hash_mask(int32_t hash_bits) { return hash_bits >= 64 ? ~0ull : hash_bits <= 0 ? 0ull : (1ull << hash_bits) - 1ull; }

// is [lo, hi) exactly `word` (n bytes)?
template <class M> DN_HD bool is_word(M &in, int64_t lo, int64_t hi, const char *word, int n)
{
    if (hi - lo != n) return false;
    for (int k = 0; k < n; k++)
        if (in.at(lo + k) != (uint32_t) (uint8_t) word[k]) return false;
    return true;
}

template <class M> DN_HD void strip(M &in, int64_t *lo, int64_t *hi)
{
    int64_t a = *lo, z = *hi;
    while (a < z && in.at(a) == ' ') a++;
    while (z > a && in.at(z - 1) == ' ') z--;
    *lo = a; *hi = z;
}

// The values of the six tags the rule reads, of attribute field [a, fe): the first piece with a tag wins, empty or not.
struct Tags {
    int64_t id_lo, id_hi, par_lo, par_hi, gname_lo, gname_hi, gene_lo, gene_hi, name_lo, name_hi, gid_lo, gid_hi;
    uint32_t seen;
};
enum { kId = 1, kParent = 2, kGeneName = 4, kGene = 8, kName = 16, kGeneId = 32 };

template <class M> DN_HD void read_tags(M &in, int64_t a, int64_t fe, Tags &T)
{
    T = Tags{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0u};
    int64_t p = a;
    for (;;) {
        int64_t q = p;
        while (q < fe && in.at(q) != ';') q++;
        int64_t lo = p, hi = q;
        strip(in, &lo, &hi);
        int64_t e = lo;
        while (e < hi && in.at(e) != '=') e++;
        int64_t t_lo = lo, t_hi = e, v_lo = e < hi ? e + 1 : hi, v_hi = hi;
        strip(in, &t_lo, &t_hi);
        strip(in, &v_lo, &v_hi);
        const uint32_t tag = is_word(in, t_lo, t_hi, "ID", 2) ? kId : is_word(in, t_lo, t_hi, "Parent", 6) ? kParent
                             : is_word(in, t_lo, t_hi, "gene_name", 9) ? kGeneName : is_word(in, t_lo, t_hi, "gene", 4) ? kGene
                             : is_word(in, t_lo, t_hi, "Name", 4) ? kName : is_word(in, t_lo, t_hi, "gene_id", 7) ? kGeneId : 0u;
        if (tag && !(T.seen & tag)) {
            T.seen |= tag;
            if (tag == kId) { T.id_lo = v_lo; T.id_hi = v_hi; }
            else if (tag == kParent) { T.par_lo = v_lo; T.par_hi = v_hi; }
            else if (tag == kGeneName) { T.gname_lo = v_lo; T.gname_hi = v_hi; }
            else if (tag == kGene) { T.gene_lo = v_lo; T.gene_hi = v_hi; }
            else if (tag == kName) { T.name_lo = v_lo; T.name_hi = v_hi; }
            else { T.gid_lo = v_lo; T.gid_hi = v_hi; }
        }
        if (q >= fe) break;
        p = q + 1;
    }
    // Parent: the first element of a comma-separated list, spaces stripped
    int64_t c = T.par_lo;
    while (c < T.par_hi && in.at(c) != ',') c++;
    T.par_hi = c;
    strip(in, &T.par_lo, &T.par_hi);
}

// The line [beg, end) of the text (without its '\n') -> kSkip, kExon (L filled), kNode (L filled), kFasta, or -(DN_GFF3_E_*).
template <class M> DN_HD int parse_line(M &in, int64_t beg, int64_t end, Line &L)
{
    if (end > beg && in.at(end - 1) == '\r') end--;
    if (end <= beg) return kSkip;
    if (in.at(beg) == '#') return is_word(in, beg, end, "##FASTA", 7) ? kFasta : kSkip;
    NineFields F;
    if (!nine_fields(in, beg, end, F)) return -DN_GFF3_E_FIELDS;
    int64_t fe = F.t8 + 1;                               // field nine ends at a further tab or at the line's end
    while (fe < end && in.at(fe) != '\t') fe++;
    Tags T;
    if (is_exon(in, F)) {
        if (!parse_uint(in, F.t3 + 1, F.t4, &L.start) || !parse_uint(in, F.t4 + 1, F.t5, &L.end)) return -DN_GFF3_E_INTEGER;
        read_tags(in, F.t8 + 1, fe, T);
        L.c_lo = beg; L.c_hi = F.t1;
        L.open = 0;
        if (T.gname_hi > T.gname_lo) { L.a_lo = T.gname_lo; L.a_hi = T.gname_hi; }
        else if (T.gene_hi > T.gene_lo) { L.a_lo = T.gene_lo; L.a_hi = T.gene_hi; }
        else if (T.par_hi > T.par_lo) { L.a_lo = T.par_lo; L.a_hi = T.par_hi; L.open = 1; }
        else if (T.gid_hi > T.gid_lo) { L.a_lo = T.gid_lo; L.a_hi = T.gid_hi; }
        else return -DN_GFF3_E_GENE;
        return kExon;
    }
    read_tags(in, F.t8 + 1, fe, T);
    if (T.id_hi <= T.id_lo) return kSkip;
    L.c_lo = T.id_lo; L.c_hi = T.id_hi;
    L.start = 0; L.end = 0;
    L.open = 0;
    if (T.gname_hi > T.gname_lo) { L.a_lo = T.gname_lo; L.a_hi = T.gname_hi; }
    else if (T.gene_hi > T.gene_lo) { L.a_lo = T.gene_lo; L.a_hi = T.gene_hi; }
    else if (T.par_hi > T.par_lo) { L.a_lo = T.par_lo; L.a_hi = T.par_hi; L.open = 1; }
    else if (T.name_hi > T.name_lo) { L.a_lo = T.name_lo; L.a_hi = T.name_hi; }
    else if (T.gid_hi > T.gid_lo) { L.a_lo = T.gid_lo; L.a_hi = T.gid_hi; }
    else { L.a_lo = T.id_lo; L.a_hi = T.id_hi; }
    return kNode;
}

// The node rows of a file in file order, and their order by (ID hash, ordinal): key[k] ascending, ord[k] the node.
struct Nodes {
    int64_t n;
    const uint64_t *key;
    const uint32_t *ord;
    const int64_t *id_beg;
    const int32_t *id_len;
    const int64_t *a_beg;
    const int32_t *a_len;
    const uint64_t *a_hash;
    const uint8_t *open;
};

// From the ID [*beg, *beg + *len) with (masked) hash *hash to the gene name: 0 and the name's span and its full hash, or
// DN_GFF3_E_PARENT / DN_GFF3_E_DEPTH.  want and have read the same text: two readers, because each caches a word.
template <class M> DN_HD int walk(M &want, M &have, const Nodes &N, int64_t *beg, int32_t *len, uint64_t *hash)
{
    int64_t w_beg = *beg;
    int32_t w_len = *len;
    uint64_t w_hash = *hash;
    for (int step = 0; step < kMaxLookups; step++) {
        int64_t a = 0, b = N.n;                         // the first entry whose key is not below w_hash
        while (a < b) {
            const int64_t mid = a + ((b - a) >> 1);
            if (N.key[mid] < w_hash) a = mid + 1; else b = mid;
        }
        int64_t found = -1;
        for (; a < N.n && N.key[a] == w_hash && found < 0; a++) {
            const int64_t k = (int64_t) N.ord[a];
            if (k >= N.n || N.id_len[k] != w_len) continue;
            const int64_t id = N.id_beg[k];
            bool same = true;
            for (int32_t j = 0; j < w_len && same; j++) same = want.at(w_beg + j) == have.at(id + j);
            if (same) found = k;
        }
        if (found < 0) return DN_GFF3_E_PARENT;
        w_beg = N.a_beg[found]; w_len = N.a_len[found]; w_hash = N.a_hash[found];
        if (!N.open[found]) {
            *beg = w_beg; *len = w_len; *hash = w_hash;
            return 0;
        }
    }
    return DN_GFF3_E_DEPTH;
}

}  // namespace gff3
}  // namespace dn

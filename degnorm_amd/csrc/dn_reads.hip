// dn_reads.hip -- per-sample chromosome coverage and gene read counts on the device.
//
// Replaces the per-read Python loop of BamReadsProcessor.chromosome_coverage_read_counts (reference reads.py:314-818).
// One chromosome per call.  The host packs the reads (positions, CIGAR bytes + offsets, pair ids) and the annotation
// (merged exon union, overlap groups with their genes' exon bounds, isolated gene spans); the device does the rest:
//
//   k_prefilter      per row: CIGAR length sum -> end_pos (:404), position pre-filter (:412-413), pair occurrence counts
//   k_pair_flag / scan / k_pair_compact      (paired) rows whose pair id occurs exactly twice, in the given row order
//                                             (:417-420); consecutive survivors form the pairs (:451)
//   k_reads          per read (or pair): CIGAR parse (:9-66), mate-2 clipping (:459-470), exon-union filter (:474-484,
//                    :499-507), overlap-group stage (:585-632), isolated-gene stage (:685-774); integer atomics for the
//                    counts, +1 / -1 events of the read's merged runs into two difference arrays
//   scans            the chromosome vector and the concatenated overlap-gene vectors (one pad slot per gene)
//   select           the chromosome vector's nonzeros -> CSR indices / values (:785-786), in position order
//
// Every accumulation is an integer atomic, so the result does not depend on the order in which reads are processed:
// two runs give bit-identical outputs.  Positions inside the kernels are int32 (the host checks chrom_len < 2^31 - 4).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"

namespace {

constexpr int kNT = 256;
constexpr int kMaxSeg = DN_READS_MAX_SEG;           // match segments per row (per mate)
constexpr int kMaxPiece = 2 * kMaxSeg + 1;          // a pair's segments plus the wrap piece of the overlap-gene index

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// Sum of all op lengths of a CIGAR string: the token grammar of the reference's regex (\d+)([A-Z]?) (:404-405).
__device__ int64_t cigar_length(const uint8_t *s, int64_t n)
{
    int64_t tot = 0, i = 0;
    while (i < n) {
        if (!is_digit(s[i])) { i++; continue; }
        int64_t len = 0;
        while (i < n && is_digit(s[i])) { len = len * 10 + (s[i] - '0'); i++; }
        tot += len;
        if (i < n && s[i] >= 'A' && s[i] <= 'Z') i++;
    }
    return tot;
}

// Match segments of one CIGAR string starting at `start` (cigar_segment_bounds, :9-66): an M op of length L gives
// [start, start + L - 1] and advances by L - 1; any other op (a digit run followed by no capital letter, e.g. '=',
// included) advances by its length, by one more when it directly follows an M.  Returns the number of M ops (0: the
// reference raises ValueError); segments beyond `cap` are counted but not stored.
__device__ int cigar_segments(const uint8_t *s, int64_t n, int64_t start, int32_t *a, int32_t *b, int cap)
{
    int nseg = 0;
    bool augment = false;
    int64_t i = 0;
    while (i < n) {
        if (!is_digit(s[i])) { i++; continue; }
        int64_t len = 0;
        while (i < n && is_digit(s[i])) { len = len * 10 + (s[i] - '0'); i++; }
        bool m = false;
        if (i < n && s[i] >= 'A' && s[i] <= 'Z') { m = s[i] == 'M'; i++; }
        if (m) {
            if (nseg < cap) { a[nseg] = (int32_t) start; b[nseg] = (int32_t) (start + len - 1); }
            nseg++;
            start += len - 1;
            augment = true;
        } else {
            start += augment ? len + 1 : len;
            augment = false;
        }
    }
    return nseg;
}

// last k in [0, n) with lo[2k] <= x, or -1 (intervals given as flat (lo, hi) pairs sorted by lo)
__device__ __forceinline__ int64_t find_le(const int64_t *iv, int64_t n, int64_t x)
{
    int64_t l = 0, h = n;                   // invariant: iv[2*(l-1)] <= x < iv[2*h]
    while (l < h) {
        const int64_t m = (l + h) >> 1;
        if (iv[2 * m] <= x) l = m + 1; else h = m;
    }
    return l - 1;
}

// [x, y] inside one interval of a merged, sorted interval list (closed bounds)
__device__ __forceinline__ bool inside(const int64_t *iv, int64_t n, int64_t x, int64_t y)
{
    const int64_t k = find_le(iv, n, x);
    return k >= 0 && y <= iv[2 * k + 1];
}

// flat view of a segment list: element 2k is a[k], 2k + 1 is b[k] (the reference's bounds list)
__device__ __forceinline__ int32_t &flat(int32_t *a, int32_t *b, int k) { return (k & 1) ? b[k >> 1] : a[k >> 1]; }

// sort pieces by start, merge overlapping / touching ones, emit +1 / -1 events into `diff` at `base` (a position is
// covered at most once per read: the reference's fancy-index += ignores duplicate indices, :617 / :773)
__device__ void emit_runs(int32_t *a, int32_t *b, int n, int *diff, int64_t base)
{
    for (int i = 1; i < n; i++) {
        const int32_t x = a[i], y = b[i];
        int j = i - 1;
        while (j >= 0 && a[j] > x) { a[j + 1] = a[j]; b[j + 1] = b[j]; j--; }
        a[j + 1] = x; b[j + 1] = y;
    }
    int i = 0;
    while (i < n) {
        int32_t lo = a[i], hi = b[i];
        i++;
        while (i < n && a[i] <= hi + 1) { if (b[i] > hi) hi = b[i]; i++; }
        atomicAdd(diff + base + lo, 1);
        atomicAdd(diff + base + hi + 1, -1);
    }
}

struct ReadsArgs {
    int32_t paired;
    int64_t n_units;                      // reads (single-end) or pairs
    const int64_t *pos, *end_pos, *cig_off;
    const uint8_t *cig;
    const int32_t *keep;                  // single-end: pre-filter flags per row
    const int32_t *rows;                  // paired: the surviving rows in order (2 per pair)
    int64_t n_exon; const int64_t *exon_iv;
    int64_t n_groups; const int64_t *group_iv; const int32_t *group_gene_off;
    const int32_t *ol_gene; const int64_t *ol_gstart0, *ol_cov_off; const int32_t *ol_exon_off; const int64_t *ol_exon;
    int64_t n_iso; const int64_t *iso_iv; const int32_t *iso_gene;
    int64_t n_iso_union; const int64_t *iso_union;
    int *counts, *ol_diff, *chrom_diff;
    unsigned long long *n_iso_reads;
    unsigned long long *err;              // first row (min over rows) [0] without M, [1] over the segment cap, [2] whose
                                          // overlap-gene index leaves [-1, L) (exons outside the gene span)
};

__global__ __launch_bounds__(kNT) void k_prefilter(int64_t n, const int64_t *__restrict__ pos, const int64_t *__restrict__ off,
                                                   const uint8_t *__restrict__ cig, int64_t keep_lo, int64_t keep_hi,
                                                   const int32_t *__restrict__ pair_id, int32_t *__restrict__ pair_cnt,
                                                   int64_t *__restrict__ end_pos, int32_t *__restrict__ keep)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT) {
        const int64_t e = pos[r] + cigar_length(cig + off[r], off[r + 1] - off[r]);
        end_pos[r] = e;
        const int32_t k = pos[r] >= keep_lo && e <= keep_hi;
        keep[r] = k;
        if (k && pair_id) atomicAdd(pair_cnt + pair_id[r], 1);
    }
}

__global__ __launch_bounds__(kNT) void k_pair_flag(int64_t n, const int32_t *__restrict__ pair_id, const int32_t *__restrict__ pair_cnt,
                                                   int32_t *__restrict__ keep)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT)
        keep[r] = keep[r] && pair_cnt[pair_id[r]] == 2;
}

__global__ __launch_bounds__(kNT) void k_pair_compact(int64_t n, const int32_t *__restrict__ keep, const int32_t *__restrict__ rank,
                                                      int32_t *__restrict__ rows)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT)
        if (keep[r]) rows[rank[r]] = (int32_t) r;
}

__global__ __launch_bounds__(kNT) void k_reads(ReadsArgs A)
{
    int32_t sa[kMaxPiece], sb[kMaxPiece];
    for (int64_t u = (int64_t) blockIdx.x * kNT + threadIdx.x; u < A.n_units; u += (int64_t) gridDim.x * kNT) {
        int64_t r2;                                          // the row whose pos / end_pos the gene stages use (:520)
        int nseg;
        if (!A.paired) {
            r2 = u;
            if (!A.keep[u]) continue;
            nseg = cigar_segments(A.cig + A.cig_off[u], A.cig_off[u + 1] - A.cig_off[u], A.pos[u], sa, sb, kMaxSeg);
            if (nseg == 0) { atomicMin(A.err + 0, (unsigned long long) u); continue; }
            if (nseg > kMaxSeg) { atomicMin(A.err + 1, (unsigned long long) u); continue; }
        } else {
            const int64_t r1 = A.rows[2 * u];
            r2 = A.rows[2 * u + 1];
            const int n1 = cigar_segments(A.cig + A.cig_off[r1], A.cig_off[r1 + 1] - A.cig_off[r1], A.pos[r1], sa, sb, kMaxSeg);
            const int n2 = cigar_segments(A.cig + A.cig_off[r2], A.cig_off[r2 + 1] - A.cig_off[r2], A.pos[r2],
                                          sa + (n1 < kMaxSeg ? n1 : kMaxSeg), sb + (n1 < kMaxSeg ? n1 : kMaxSeg), kMaxSeg);
            if (n1 == 0 || n2 == 0) { atomicMin(A.err + 0, (unsigned long long) (n1 == 0 ? r1 : r2)); continue; }
            if (n1 > kMaxSeg || n2 > kMaxSeg) { atomicMin(A.err + 1, (unsigned long long) (n1 > kMaxSeg ? r1 : r2)); continue; }
            // mate 2 clipped against mate 1's extent (:460-467)
            int32_t mn1 = sa[0], mx1 = sa[0], mx2 = sa[n1];
            for (int k = 0; k < 2 * n1; k++) { const int32_t v = flat(sa, sb, k); mn1 = v < mn1 ? v : mn1; mx1 = v > mx1 ? v : mx1; }
            int32_t *a2 = sa + n1, *b2 = sb + n1;
            for (int k = 0; k < 2 * n2; k++) { const int32_t v = flat(a2, b2, k); mx2 = v > mx2 ? v : mx2; }
            if (mx2 >= mx1) {
                for (int k = 0; k < 2 * n2; k++) { int32_t &v = flat(a2, b2, k); if (v <= mx1) v = mx1 + 1; }
            } else {
                for (int k = 0; k < 2 * n2; k++) { int32_t &v = flat(a2, b2, k); if (v >= mn1) v = mn1 - 1; }
                for (int k = 1; k < 2 * n2; k++) {               // bounds_2.sort(): the flat list, then re-paired
                    const int32_t v = flat(a2, b2, k);
                    int j = k - 1;
                    while (j >= 0 && flat(a2, b2, j) > v) { flat(a2, b2, j + 1) = flat(a2, b2, j); j--; }
                    flat(a2, b2, j + 1) = v;
                }
            }
            nseg = n1 + n2;
        }
        // exon-union filter: every non-empty segment inside one merged exon interval; an empty one (end < start)
        // passes like the reference's empty slice.  A bound below 0 (a clipped mate at position 0) drops the read.
        bool drop = false;
        for (int k = 0; k < nseg && !drop; k++) {
            if (sa[k] < 0 || sb[k] < 0) drop = true;
            else if (sb[k] >= sa[k] && !inside(A.exon_iv, A.n_exon, sa[k], sb[k])) drop = true;
        }
        if (drop) continue;
        const int64_t p = A.pos[r2], e = A.end_pos[r2];
        // overlap-group stage: the one group whose span holds [pos, end_pos]; full inclusion against each of its genes
        const int64_t g = A.n_groups > 0 ? find_le(A.group_iv, A.n_groups, p) : -1;
        if (g >= 0 && e <= A.group_iv[2 * g + 1]) {
            int caught = 0, who = -1;
            for (int q = A.group_gene_off[g]; q < A.group_gene_off[g + 1] && caught < 2; q++) {
                bool all = true;
                for (int k = 0; k < nseg && all; k++) {
                    bool seg = false;
                    for (int x = A.ol_exon_off[q]; x < A.ol_exon_off[q + 1]; x++)
                        if (sa[k] >= A.ol_exon[2 * x] && sb[k] <= A.ol_exon[2 * x + 1]) { seg = true; break; }
                    all = seg;
                }
                if (all) { caught++; who = q; }
            }
            if (caught >= 2) continue;
            if (caught == 1) {
                atomicAdd(A.counts + A.ol_gene[who], 1);
                // index = position - gene_start0 - 1 (:615-616); -1 wraps to the last element of the span vector
                const int32_t sh = (int32_t) (A.ol_gstart0[who] + 1);
                const int32_t len = (int32_t) (A.ol_cov_off[who + 1] - A.ol_cov_off[who] - 1);
                int np = 0;
                bool wrap = false;
                for (int k = 0; k < nseg; k++) {
                    if (sb[k] < sa[k]) continue;
                    int32_t lo = sa[k] - sh, hi = sb[k] - sh;
                    if (lo < -1) { atomicMin(A.err + 2, (unsigned long long) r2); lo = -1; }
                    if (lo < 0) { wrap = true; lo = 0; }
                    if (hi >= len) { atomicMin(A.err + 2, (unsigned long long) r2); hi = len - 1; }
                    if (hi >= lo) { sa[np] = lo; sb[np] = hi; np++; }
                }
                if (wrap) { sa[np] = len - 1; sb[np] = len - 1; np++; }
                emit_runs(sa, sb, np, A.ol_diff, A.ol_cov_off[who]);
                continue;
            }
        }
        // isolated-gene stage: [pos, end_pos] inside the union of isolated gene spans, gene = the span holding pos
        if (A.n_iso == 0 || !inside(A.iso_union, A.n_iso_union, p, e)) continue;
        const int64_t ig = find_le(A.iso_iv, A.n_iso, p);
        if (ig < 0 || p > A.iso_iv[2 * ig + 1]) continue;
        atomicAdd(A.counts + A.iso_gene[ig], 1);
        atomicAdd(A.n_iso_reads, 1ull);
        int np = 0;
        for (int k = 0; k < nseg; k++)
            if (sb[k] >= sa[k]) { sa[np] = sa[k]; sb[np] = sb[k]; np++; }
        emit_runs(sa, sb, np, A.chrom_diff, 0);
    }
}

__global__ __launch_bounds__(kNT) void k_gather_csr(int64_t n, const int32_t *__restrict__ idx, const int *__restrict__ cov,
                                                    int64_t *__restrict__ val)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) val[i] = cov[idx[i]];
}

__global__ __launch_bounds__(kNT) void k_widen(int64_t n, const int *__restrict__ x, int64_t *__restrict__ y)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) y[i] = x[i];
}

__global__ __launch_bounds__(kNT) void k_cigar_debug(int64_t n, const int64_t *__restrict__ pos, const int64_t *__restrict__ off,
                                                     const uint8_t *__restrict__ cig, int32_t max_seg, int32_t *__restrict__ nseg,
                                                     int64_t *__restrict__ bounds, int64_t *__restrict__ end_pos)
{
    int32_t a[kMaxSeg], b[kMaxSeg];
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT) {
        const int k = cigar_segments(cig + off[r], off[r + 1] - off[r], pos[r], a, b, kMaxSeg);
        end_pos[r] = pos[r] + cigar_length(cig + off[r], off[r + 1] - off[r]);
        nseg[r] = k == 0 ? 0 : (k > max_seg || k > kMaxSeg) ? -1 : k;
        if (nseg[r] > 0)
            for (int j = 0; j < k; j++) { bounds[(int64_t) r * 2 * max_seg + 2 * j] = a[j]; bounds[(int64_t) r * 2 * max_seg + 2 * j + 1] = b[j]; }
    }
}

struct NonZero {
    const int *cov;
    __host__ __device__ bool operator()(const int32_t &i) const { return cov[i] != 0; }
};

thread_local std::string g_reads_err;

inline unsigned grid_for(int64_t n) { const int64_t g = (n + kNT - 1) / kNT; return (unsigned) (g < 1 ? 1 : g > 65536 ? 65536 : g); }

// n elements and 16 bytes of slack
template <class T> hipError_t alloc_padded(dn::DeviceBuffer<T> &b, size_t n) { return b.alloc(n * sizeof(T) + 16); }

}  // namespace

#define RD_TRY(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) { g_reads_err = std::string(#expr) + ": " + hipGetErrorString(e_); rc = DN_E_HIP; goto done; } \
    } while (0)

extern "C" const char *dn_reads_last_error(void) { return g_reads_err.c_str(); }

extern "C" int dn_read_coverage(int device, int32_t paired, int64_t n_rows, const int64_t *pos, const int64_t *cigar_off,
                                const uint8_t *cigar, const int32_t *pair_id, int64_t n_pair_ids,
                                int64_t chrom_len, int64_t keep_lo, int64_t keep_hi,
                                int64_t n_exon, const int64_t *exon_iv,
                                int64_t n_groups, const int64_t *group_iv, const int32_t *group_gene_off,
                                const int32_t *ol_gene, const int64_t *ol_gene_start0, const int64_t *ol_cov_off,
                                const int32_t *ol_exon_off, const int64_t *ol_exon_bounds,
                                int64_t n_iso, const int64_t *iso_iv, const int32_t *iso_gene,
                                int64_t n_iso_union, const int64_t *iso_union,
                                int64_t n_genes, int64_t *counts, int64_t *ol_cov,
                                int64_t csr_cap, int64_t *nnz, int32_t *csr_idx, int64_t *csr_val,
                                int64_t *n_isolated_reads, double *device_ms)
{
    int rc = DN_OK;
    g_reads_err.clear();
    if (n_rows < 0 || n_rows > INT32_MAX - 1 || chrom_len <= 0 || chrom_len > INT32_MAX - 4 || n_exon < 0 || n_groups < 0 || n_iso < 0 || n_iso_union < 0 ||
        n_genes < 0 || !counts || !nnz || !n_isolated_reads || (paired && n_rows > 0 && (!pair_id || n_pair_ids < 1)) ||
        (n_rows > 0 && (!pos || !cigar_off || !cigar)) || (n_groups > 0 && (!group_iv || !group_gene_off || !ol_cov || !ol_cov_off)) ||
        (n_iso > 0 && (!iso_iv || !iso_gene || !iso_union)) || csr_cap < 0 || (csr_cap > 0 && (!csr_idx || !csr_val))) {
        g_reads_err = "dn_read_coverage: bad argument";
        return DN_E_INVALID;
    }
    if (paired)
        for (int64_t r = 0; r < n_rows; r++)
            if (pair_id[r] < 0 || pair_id[r] >= n_pair_ids) { g_reads_err = "dn_read_coverage: pair id out of range"; return DN_E_INVALID; }
    const int64_t n_ol = n_groups > 0 ? group_gene_off[n_groups] : 0;
    const int64_t ol_total = n_ol > 0 ? ol_cov_off[n_ol] : 0;
    // every index the kernels follow stays inside its array
    for (int64_t g = 0; g < n_groups; g++)
        if (group_gene_off[g] < 0 || group_gene_off[g + 1] < group_gene_off[g]) { g_reads_err = "dn_read_coverage: bad group_gene_off"; return DN_E_INVALID; }
    for (int64_t q = 0; q < n_ol; q++)
        if (ol_gene[q] < 0 || ol_gene[q] >= n_genes || ol_cov_off[q + 1] - ol_cov_off[q] < 2 || ol_exon_off[q + 1] < ol_exon_off[q] ||
            (q == 0 && (ol_cov_off[0] != 0 || ol_exon_off[0] != 0))) { g_reads_err = "dn_read_coverage: bad overlap-gene tables"; return DN_E_INVALID; }
    for (int64_t k = 0; k < n_iso; k++)
        if (iso_gene[k] < 0 || iso_gene[k] >= n_genes) { g_reads_err = "dn_read_coverage: bad iso_gene"; return DN_E_INVALID; }
    for (int64_t k = 0; k < n_exon; k++)
        if (exon_iv[2 * k] < 0 || exon_iv[2 * k + 1] >= chrom_len) { g_reads_err = "dn_read_coverage: exon union outside the chromosome"; return DN_E_INVALID; }
    const int64_t n_ol_exon = n_ol > 0 ? ol_exon_off[n_ol] : 0;
    const int64_t n_bytes = n_rows > 0 ? cigar_off[n_rows] : 0;
    dn::DeviceBuffer<int64_t> d_pos, d_off, d_end, d_exon, d_giv, d_gs0, d_coff, d_oex, d_iiv, d_iu;
    dn::DeviceBuffer<int64_t> d_val64, d_csr_val;
    dn::DeviceBuffer<uint8_t> d_cig;
    dn::DeviceBuffer<int32_t> d_pid, d_pcnt, d_rank, d_rows, d_keep, d_ggo, d_olg, d_oxo, d_ig, d_csr_idx;
    dn::DeviceBuffer<int> d_counts, d_oldiff, d_olcov, d_cdiff, d_ccov, d_nsel;
    dn::DeviceBuffer<unsigned long long> d_niso, d_err;
    std::vector<dn::DeviceBuffer<uint8_t>> tmp;     // scan / select scratch: a larger one is added when a call needs more
    void *d_tmp = nullptr;                           // the latest of them
    dn::Stream st;
    dn::Event e0, e1;
    size_t tmp_bytes = 0, need = 0;
    int64_t n_units = 0;
    unsigned long long h_err[3], h_niso = 0;
    int h_nsel = 0;
    int32_t survivors = 0;
    std::vector<int> h_counts(n_genes > 0 ? n_genes : 1);

    RD_TRY(hipSetDevice(device));
    RD_TRY(st.create(hipStreamCreate));
    RD_TRY(e0.create(hipEventCreate));
    RD_TRY(e1.create(hipEventCreate));
    RD_TRY(alloc_padded(d_pos, n_rows)); RD_TRY(alloc_padded(d_off, n_rows + 1)); RD_TRY(alloc_padded(d_end, n_rows));
    RD_TRY(alloc_padded(d_cig, n_bytes)); RD_TRY(alloc_padded(d_keep, n_rows + 1));
    RD_TRY(alloc_padded(d_exon, 2 * n_exon)); RD_TRY(alloc_padded(d_giv, 2 * n_groups)); RD_TRY(alloc_padded(d_ggo, n_groups + 1));
    RD_TRY(alloc_padded(d_olg, n_ol)); RD_TRY(alloc_padded(d_gs0, n_ol)); RD_TRY(alloc_padded(d_coff, n_ol + 1));
    RD_TRY(alloc_padded(d_oxo, n_ol + 1)); RD_TRY(alloc_padded(d_oex, 2 * n_ol_exon));
    RD_TRY(alloc_padded(d_iiv, 2 * n_iso)); RD_TRY(alloc_padded(d_ig, n_iso)); RD_TRY(alloc_padded(d_iu, 2 * n_iso_union));
    RD_TRY(alloc_padded(d_counts, n_genes)); RD_TRY(alloc_padded(d_oldiff, ol_total)); RD_TRY(alloc_padded(d_olcov, ol_total));
    RD_TRY(alloc_padded(d_val64, ol_total));
    RD_TRY(alloc_padded(d_cdiff, chrom_len + 1)); RD_TRY(alloc_padded(d_ccov, chrom_len + 1));
    RD_TRY(alloc_padded(d_csr_idx, chrom_len)); RD_TRY(alloc_padded(d_csr_val, chrom_len)); RD_TRY(alloc_padded(d_nsel, 1));
    RD_TRY(alloc_padded(d_niso, 1)); RD_TRY(alloc_padded(d_err, 3));
    if (paired) {
        RD_TRY(alloc_padded(d_pid, n_rows)); RD_TRY(alloc_padded(d_pcnt, n_pair_ids)); RD_TRY(alloc_padded(d_rank, n_rows + 1));
        RD_TRY(alloc_padded(d_rows, n_rows));
    }
#define H2D(d, h, n) do { if ((n) > 0) RD_TRY(hipMemcpyAsync(d, h, sizeof(*(d)) * (size_t) (n), hipMemcpyHostToDevice, st)); } while (0)
    H2D(d_pos, pos, n_rows); H2D(d_off, cigar_off, n_rows > 0 ? n_rows + 1 : 0); H2D(d_cig, cigar, n_bytes);
    H2D(d_exon, exon_iv, 2 * n_exon); H2D(d_giv, group_iv, 2 * n_groups); H2D(d_ggo, group_gene_off, n_groups > 0 ? n_groups + 1 : 0);
    H2D(d_olg, ol_gene, n_ol); H2D(d_gs0, ol_gene_start0, n_ol); H2D(d_coff, ol_cov_off, n_ol > 0 ? n_ol + 1 : 0);
    H2D(d_oxo, ol_exon_off, n_ol > 0 ? n_ol + 1 : 0); H2D(d_oex, ol_exon_bounds, 2 * n_ol_exon);
    H2D(d_iiv, iso_iv, 2 * n_iso); H2D(d_ig, iso_gene, n_iso); H2D(d_iu, iso_union, 2 * n_iso_union);
    if (paired) H2D(d_pid, pair_id, n_rows);
#undef H2D
    RD_TRY(hipEventRecord(e0, st));
    RD_TRY(hipMemsetAsync(d_counts, 0, sizeof(int) * (size_t) (n_genes > 0 ? n_genes : 1), st));
    RD_TRY(hipMemsetAsync(d_oldiff, 0, sizeof(int) * (size_t) (ol_total > 0 ? ol_total : 1), st));
    RD_TRY(hipMemsetAsync(d_cdiff, 0, sizeof(int) * (size_t) (chrom_len + 1), st));
    RD_TRY(hipMemsetAsync(d_niso, 0, sizeof(unsigned long long), st));
    RD_TRY(hipMemsetAsync(d_err, 0xff, 3 * sizeof(unsigned long long), st));
    if (paired) RD_TRY(hipMemsetAsync(d_pcnt, 0, sizeof(int32_t) * (size_t) n_pair_ids, st));
    if (n_rows > 0) {
        hipLaunchKernelGGL(k_prefilter, dim3(grid_for(n_rows)), dim3(kNT), 0, st, n_rows, d_pos, d_off, d_cig, keep_lo, keep_hi,
                           paired ? d_pid.get() : (const int32_t *) nullptr, d_pcnt, d_end, d_keep);
        RD_TRY(hipGetLastError());
        n_units = n_rows;
        if (paired) {
            hipLaunchKernelGGL(k_pair_flag, dim3(grid_for(n_rows)), dim3(kNT), 0, st, n_rows, d_pid, d_pcnt, d_keep);
            RD_TRY(hipGetLastError());
            // exclusive rank of every surviving row; rank[n_rows] is the number of survivors
            RD_TRY(hipMemsetAsync(d_keep + n_rows, 0, sizeof(int32_t), st));       // keep[n_rows] = 0: rank[n_rows] = #survivors
            RD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_keep.get(), d_rank.get(), (int) n_rows + 1, st));
            if (need > tmp_bytes) { tmp.emplace_back(); RD_TRY(alloc_padded(tmp.back(), need)); d_tmp = tmp.back(); tmp_bytes = need; }
            RD_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, need, d_keep.get(), d_rank.get(), (int) n_rows + 1, st));
            hipLaunchKernelGGL(k_pair_compact, dim3(grid_for(n_rows)), dim3(kNT), 0, st, n_rows, d_keep, d_rank, d_rows);
            RD_TRY(hipGetLastError());
            RD_TRY(hipMemcpyAsync(&survivors, d_rank + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            RD_TRY(hipStreamSynchronize(st));
            n_units = survivors / 2;
        }
        if (n_units > 0) {
            ReadsArgs A;
            A.paired = paired; A.n_units = n_units; A.pos = d_pos; A.end_pos = d_end; A.cig_off = d_off; A.cig = d_cig;
            A.keep = d_keep; A.rows = d_rows;
            A.n_exon = n_exon; A.exon_iv = d_exon; A.n_groups = n_groups; A.group_iv = d_giv; A.group_gene_off = d_ggo;
            A.ol_gene = d_olg; A.ol_gstart0 = d_gs0; A.ol_cov_off = d_coff; A.ol_exon_off = d_oxo; A.ol_exon = d_oex;
            A.n_iso = n_iso; A.iso_iv = d_iiv; A.iso_gene = d_ig; A.n_iso_union = n_iso_union; A.iso_union = d_iu;
            A.counts = d_counts; A.ol_diff = d_oldiff; A.chrom_diff = d_cdiff; A.n_iso_reads = d_niso; A.err = d_err;
            hipLaunchKernelGGL(k_reads, dim3(grid_for(n_units)), dim3(kNT), 0, st, A);
            RD_TRY(hipGetLastError());
        }
    }
    // difference arrays -> coverage
    need = 0;
    RD_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, need, d_cdiff.get(), d_ccov.get(), (int) chrom_len, st));
    if (need > tmp_bytes) { tmp.emplace_back(); RD_TRY(alloc_padded(tmp.back(), need)); d_tmp = tmp.back(); tmp_bytes = need; }
    RD_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, need, d_cdiff.get(), d_ccov.get(), (int) chrom_len, st));
    if (ol_total > 0) {
        need = 0;
        RD_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, need, d_oldiff.get(), d_olcov.get(), (int) ol_total, st));
        if (need > tmp_bytes) { tmp.emplace_back(); RD_TRY(alloc_padded(tmp.back(), need)); d_tmp = tmp.back(); tmp_bytes = need; }
        RD_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, need, d_oldiff.get(), d_olcov.get(), (int) ol_total, st));
        hipLaunchKernelGGL(k_widen, dim3(grid_for(ol_total)), dim3(kNT), 0, st, ol_total, d_olcov, d_val64);
        RD_TRY(hipGetLastError());
    }
    // chromosome vector -> CSR (positions ascending)
    {
        hipcub::CountingInputIterator<int32_t> ids(0);
        NonZero nz{d_ccov.get()};
        need = 0;
        RD_TRY(hipcub::DeviceSelect::If(nullptr, need, ids, d_csr_idx.get(), d_nsel.get(), (int) chrom_len, nz, st));
        if (need > tmp_bytes) { tmp.emplace_back(); RD_TRY(alloc_padded(tmp.back(), need)); d_tmp = tmp.back(); tmp_bytes = need; }
        RD_TRY(hipcub::DeviceSelect::If(d_tmp, need, ids, d_csr_idx.get(), d_nsel.get(), (int) chrom_len, nz, st));
    }
    RD_TRY(hipMemcpyAsync(&h_nsel, d_nsel, sizeof(int), hipMemcpyDeviceToHost, st));
    RD_TRY(hipMemcpyAsync(h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost, st));
    RD_TRY(hipMemcpyAsync(&h_niso, d_niso, sizeof(h_niso), hipMemcpyDeviceToHost, st));
    RD_TRY(hipStreamSynchronize(st));
    if (h_nsel > 0) {
        hipLaunchKernelGGL(k_gather_csr, dim3(grid_for(h_nsel)), dim3(kNT), 0, st, (int64_t) h_nsel, d_csr_idx, d_ccov, d_csr_val);
        RD_TRY(hipGetLastError());
    }
    RD_TRY(hipEventRecord(e1, st));
    if (h_err[0] != ~0ull) {
        const int64_t r = (int64_t) h_err[0];
        g_reads_err = "CIGAR string " + std::string((const char *) cigar + cigar_off[r], (size_t) (cigar_off[r + 1] - cigar_off[r])) +
                      " has no matching region.";
        rc = DN_E_INVALID;
        goto done;
    }
    if (h_err[1] != ~0ull) {
        const int64_t r = (int64_t) h_err[1];
        g_reads_err = "CIGAR string " + std::string((const char *) cigar + cigar_off[r], (size_t) (cigar_off[r + 1] - cigar_off[r])) +
                      " has more than " + std::to_string(kMaxSeg) + " match segments (DN_READS_MAX_SEG)";
        rc = DN_E_UNSUPPORTED;
        goto done;
    }
    if (h_err[2] != ~0ull) {
        g_reads_err = "an overlap gene's exons reach past its gene span (row " + std::to_string(h_err[2]) + ")";
        rc = DN_E_INVALID;
        goto done;
    }
    if (h_nsel > csr_cap) {
        g_reads_err = "dn_read_coverage: " + std::to_string(h_nsel) + " nonzeros exceed csr_cap " + std::to_string(csr_cap);
        rc = DN_E_INVALID;
        goto done;
    }
    *nnz = h_nsel;
    *n_isolated_reads = (int64_t) h_niso;
    if (h_nsel > 0) {
        RD_TRY(hipMemcpyAsync(csr_idx, d_csr_idx, sizeof(int32_t) * (size_t) h_nsel, hipMemcpyDeviceToHost, st));
        RD_TRY(hipMemcpyAsync(csr_val, d_csr_val, sizeof(int64_t) * (size_t) h_nsel, hipMemcpyDeviceToHost, st));
    }
    if (ol_total > 0) RD_TRY(hipMemcpyAsync(ol_cov, d_val64, sizeof(int64_t) * (size_t) ol_total, hipMemcpyDeviceToHost, st));
    if (n_genes > 0) RD_TRY(hipMemcpyAsync(h_counts.data(), d_counts, sizeof(int) * (size_t) n_genes, hipMemcpyDeviceToHost, st));
    RD_TRY(hipStreamSynchronize(st));
    for (int64_t k = 0; k < n_genes; k++) counts[k] = h_counts[k];
    if (device_ms) { float ms = 0.f; RD_TRY(hipEventElapsedTime(&ms, e0, e1)); *device_ms = ms; }
done:
    if (st) (void) hipStreamSynchronize(st);
    return rc;
}

extern "C" int dn_reads_cigar_bounds(int device, int64_t n, const int64_t *pos, const int64_t *cigar_off, const uint8_t *cigar,
                                     int32_t max_seg, int32_t *nseg, int64_t *bounds, int64_t *end_pos)
{
    int rc = DN_OK;
    g_reads_err.clear();
    if (n < 0 || max_seg < 1 || max_seg > kMaxSeg || (n > 0 && (!pos || !cigar_off || !cigar || !nseg || !bounds || !end_pos))) {
        g_reads_err = "dn_reads_cigar_bounds: bad argument";
        return DN_E_INVALID;
    }
    if (n == 0) return DN_OK;
    dn::DeviceBuffer<int64_t> d_pos, d_off, d_b, d_end;
    dn::DeviceBuffer<uint8_t> d_cig;
    dn::DeviceBuffer<int32_t> d_n;
    dn::Stream st;
    const int64_t n_bytes = cigar_off[n];
    RD_TRY(hipSetDevice(device));
    RD_TRY(st.create(hipStreamCreate));
    RD_TRY(alloc_padded(d_pos, n)); RD_TRY(alloc_padded(d_off, n + 1)); RD_TRY(alloc_padded(d_cig, n_bytes)); RD_TRY(alloc_padded(d_n, n));
    RD_TRY(alloc_padded(d_b, n * 2 * max_seg)); RD_TRY(alloc_padded(d_end, n));
    RD_TRY(hipMemcpyAsync(d_pos, pos, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, st));
    RD_TRY(hipMemcpyAsync(d_off, cigar_off, sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice, st));
    if (n_bytes > 0) RD_TRY(hipMemcpyAsync(d_cig, cigar, (size_t) n_bytes, hipMemcpyHostToDevice, st));
    RD_TRY(hipMemsetAsync(d_b, 0, sizeof(int64_t) * (size_t) (n * 2 * max_seg), st));
    hipLaunchKernelGGL(k_cigar_debug, dim3(grid_for(n)), dim3(kNT), 0, st, n, d_pos, d_off, d_cig, max_seg, d_n, d_b, d_end);
    RD_TRY(hipGetLastError());
    RD_TRY(hipMemcpyAsync(nseg, d_n, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
    RD_TRY(hipMemcpyAsync(bounds, d_b, sizeof(int64_t) * (size_t) (n * 2 * max_seg), hipMemcpyDeviceToHost, st));
    RD_TRY(hipMemcpyAsync(end_pos, d_end, sizeof(int64_t) * (size_t) n, hipMemcpyDeviceToHost, st));
    RD_TRY(hipStreamSynchronize(st));
done:
    if (st) (void) hipStreamSynchronize(st);
    return rc;
}

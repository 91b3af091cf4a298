// dn_reads.hip -- per-sample chromosome coverage and gene read counts on the device.
//
// Replaces the per-read Python loop of BamReadsProcessor.chromosome_coverage_read_counts (reference reads.py:314-818).
// One chromosome per call.  The host packs the reads (positions, CIGAR bytes + offsets, pair ids) and the annotation
// (merged exon union, overlap groups with their genes' exon bounds, isolated gene spans); the device does the rest:
//
//   k_prefilter      per row: CIGAR length sum -> end_pos (:404), position pre-filter (:412-413), pair occurrence counts
//   k_pair_flag / scan / k_pair_compact      (paired) rows whose pair id occurs exactly twice, in the given row order
//                                             (:417-420); consecutive survivors form the pairs (:451).  Pairing by FLAG: twice,
//                                             once as a first mate (0x40) and once as a last one (MateBits)
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
#include <string.h>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_inflate.hpp"
#include "dn_frame.hpp"
#include "dn_bam_record.hpp"
#include "dn_pair.hpp"

namespace {

constexpr int kNT = 256;
constexpr int64_t kGridCap = 65536;
constexpr int kMaxSeg = DN_READS_MAX_SEG;           // match segments per row (per mate)
constexpr int kMaxPiece = 2 * kMaxSeg + 1;          // a pair's segments plus the wrap piece of the overlap-gene index

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// CIGAR sources.  A row's CIGAR is read as a sequence of tokens (length, is-M); the stages below are written once against
// a source type and instantiated for two of them:
//   StrCigars   ASCII strings cigar[off[r] .. off[r+1]) in the token grammar of the reference's regex (\d+)([A-Z]?):
//               text that is not a digit run is skipped, a digit run is one token, M only when the capital letter 'M'
//               directly follows it (:9-66, :404-405)
//   BamCigars   BAM's binary ops (len << 4 | op) ops[beg[r] .. beg[r] + cnt[r]): only op 0 (M) is a match; every other op,
//               = (7) and X (8) included, is "other" -- what pysam's cigarstring gives the regex
struct StrTokens {
    const uint8_t *s;
    int64_t n, i;
    __device__ bool next(int64_t &len, bool &m)
    {
        while (i < n && !is_digit(s[i])) i++;
        if (i >= n) return false;
        len = 0;
        while (i < n && is_digit(s[i])) { len = len * 10 + (s[i] - '0'); i++; }
        m = false;
        if (i < n && s[i] >= 'A' && s[i] <= 'Z') { m = s[i] == 'M'; i++; }
        return true;
    }
};

struct BamTokens {
    const uint32_t *p;
    int64_t n, i;
    __device__ bool next(int64_t &len, bool &m)
    {
        if (i >= n) return false;
        const uint32_t v = p[i++];
        len = v >> 4;
        m = (v & 15u) == 0;
        return true;
    }
};

struct StrCigars {
    const int64_t *off;
    const uint8_t *cig;
    __device__ StrTokens row(int64_t r) const { return StrTokens{cig + off[r], off[r + 1] - off[r], 0}; }
};

struct BamCigars {
    const int64_t *beg;
    const int32_t *cnt;
    const uint32_t *ops;
    __device__ BamTokens row(int64_t r) const { return BamTokens{ops + beg[r], cnt[r], 0}; }
};

// Sum of all op lengths of a CIGAR (:404-405).
template <class T> __device__ int64_t cigar_length(T t)
{
    int64_t tot = 0, len;
    bool m;
    while (t.next(len, m)) tot += len;
    return tot;
}

// Match segments of one CIGAR starting at `start` (cigar_segment_bounds, :9-66): an M op of length L gives
// [start, start + L - 1] and advances by L - 1; any other op advances by its length, by one more when it directly follows
// an M.  Returns the number of M ops (0: the reference raises ValueError); segments beyond `cap` are counted but not stored.
template <class T> __device__ int cigar_segments(T t, int64_t start, int32_t *a, int32_t *b, int cap)
{
    int nseg = 0;
    bool augment = false;
    int64_t len;
    bool m;
    while (t.next(len, m)) {
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

template <class C> struct ReadsArgs {
    int32_t paired;
    int64_t n_units;                      // reads (single-end) or pairs
    const int64_t *pos, *end_pos;
    C cig;
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

// Pairing by FLAG: the FLAG of the row taken at position r is flag[order[r]].  A pair is then a key with two rows of which
// one is a first mate (0x40): every row adds 1 to its key's counter and a first mate kMateFirst besides, and the counter
// of a pair -- and of nothing else, among at most kMateRowsMax rows: the sum is taken modulo 2^32, and rows = 2 (mod 2^30)
// leaves rows = 2 -- reads kMatePair.  The name rule (flag == NULL) adds 1 per row and a pair reads 2.
struct MateBits {
    const uint16_t *flag = nullptr;
    const int32_t *order = nullptr;
};
constexpr int32_t kMateFirst = 1 << 30, kMatePair = 2 | kMateFirst;
constexpr int64_t kMateRowsMax = (int64_t) 1 << 30;

// Strand-specific counting: the sense of the row taken at position r is sense[order ? order[r] : r], and the call counts
// the rows whose sense is `want` (dn::kSensePlus or dn::kSenseMinus).
struct StrandSel {
    const uint8_t *sense = nullptr;
    const int32_t *order = nullptr;
    uint8_t want = 0;
};

// STRAND: the position pre-filter also asks for the sense `sel.want`; a row of the other sense is dropped before it is
// counted for its pair, so a pair whose mates disagree leaves one row here and is no pair.  The instances without it take
// no selector and are the kernels of the unstranded call.
template <class C, bool MATES, bool STRAND, class... Sel>
__global__ __launch_bounds__(kNT) void k_prefilter(int64_t n, const int64_t *__restrict__ pos, C cig, int64_t keep_lo, int64_t keep_hi,
                                                   const int32_t *__restrict__ pair_id, int32_t *__restrict__ pair_cnt, MateBits mates,
                                                   int64_t *__restrict__ end_pos, int32_t *__restrict__ keep, Sel... sel)
{
    static_assert(sizeof...(Sel) == (STRAND ? 1 : 0), "a stranded instance takes one StrandSel, the others none");
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT) {
        const int64_t e = pos[r] + cigar_length(cig.row(r));
        end_pos[r] = e;
        int32_t k = pos[r] >= keep_lo && e <= keep_hi;
        if constexpr (STRAND) {
            const StrandSel s{sel...};
            k = k && s.sense[s.order ? s.order[r] : r] == s.want;
        }
        keep[r] = k;
        if (MATES) {
            if (k) atomicAdd((unsigned int *) pair_cnt + pair_id[r], (mates.flag[mates.order[r]] & dn::kFlagFirst) ? 1u | (unsigned int) kMateFirst : 1u);
        } else if (k && pair_id) {
            atomicAdd(pair_cnt + pair_id[r], 1);
        }
    }
}

__global__ __launch_bounds__(kNT) void k_pair_flag(int64_t n, const int32_t *__restrict__ pair_id, const int32_t *__restrict__ pair_cnt,
                                                   int32_t is_pair, int32_t *__restrict__ keep)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT)
        keep[r] = keep[r] && pair_cnt[pair_id[r]] == is_pair;
}

__global__ __launch_bounds__(kNT) void k_pair_compact(int64_t n, const int32_t *__restrict__ keep, const int32_t *__restrict__ rank,
                                                      int32_t *__restrict__ rows)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT)
        if (keep[r]) rows[rank[r]] = (int32_t) r;
}

template <class C> __global__ __launch_bounds__(kNT) void k_reads(ReadsArgs<C> A)
{
    int32_t sa[kMaxPiece], sb[kMaxPiece];
    for (int64_t u = (int64_t) blockIdx.x * kNT + threadIdx.x; u < A.n_units; u += (int64_t) gridDim.x * kNT) {
        int64_t r2;                                          // the row whose pos / end_pos the gene stages use (:520)
        int nseg;
        if (!A.paired) {
            r2 = u;
            if (!A.keep[u]) continue;
            nseg = cigar_segments(A.cig.row(u), A.pos[u], sa, sb, kMaxSeg);
            if (nseg == 0) { atomicMin(A.err + 0, (unsigned long long) u); continue; }
            if (nseg > kMaxSeg) { atomicMin(A.err + 1, (unsigned long long) u); continue; }
        } else {
            const int64_t r1 = A.rows[2 * u];
            r2 = A.rows[2 * u + 1];
            const int n1 = cigar_segments(A.cig.row(r1), A.pos[r1], sa, sb, kMaxSeg);
            const int n2 = cigar_segments(A.cig.row(r2), A.pos[r2],
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
        // passes like the reference's empty slice.  A bound below 0 (a zero-length M at position 0, or a mate clipped
        // below a mate at position 0) drops the read or pair.
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

template <class C>
__global__ __launch_bounds__(kNT) void k_cigar_debug(int64_t n, const int64_t *__restrict__ pos, C cig, int32_t max_seg, int32_t *__restrict__ nseg,
                                                     int64_t *__restrict__ bounds, int64_t *__restrict__ end_pos)
{
    int32_t a[kMaxSeg], b[kMaxSeg];
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT) {
        const int k = cigar_segments(cig.row(r), pos[r], a, b, kMaxSeg);
        end_pos[r] = pos[r] + cigar_length(cig.row(r));
        nseg[r] = k == 0 ? 0 : (k > max_seg || k > kMaxSeg) ? -1 : k;
        if (nseg[r] > 0)
            for (int j = 0; j < k; j++) { bounds[(int64_t) r * 2 * max_seg + 2 * j] = a[j]; bounds[(int64_t) r * 2 * max_seg + 2 * j + 1] = b[j]; }
    }
}

struct NonZero {
    const int *cov;
    __host__ __device__ bool operator()(const int32_t &i) const { return cov[i] != 0; }
};

// k_cigar_debug on n rows whose CIGARs are already on the device (`cig`); pos and the outputs are host arrays.
template <class C>
int cigar_debug(hipStream_t st, int64_t n, const int64_t *pos, C cig, int32_t max_seg, int32_t *nseg, int64_t *bounds, int64_t *end_pos)
{
    dn::DeviceBuffer<int64_t> d_pos, d_b, d_end;
    dn::DeviceBuffer<int32_t> d_n;
    return dn::synced(st, [&]() -> int {
        DN_TRY(alloc_padded(d_pos, n)); DN_TRY(alloc_padded(d_n, n)); DN_TRY(alloc_padded(d_b, n * 2 * max_seg)); DN_TRY(alloc_padded(d_end, n));
        DN_TRY(hipMemcpyAsync(d_pos, pos, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemsetAsync(d_b, 0, sizeof(int64_t) * (size_t) (n * 2 * max_seg), st));
        hipLaunchKernelGGL(k_cigar_debug<C>, dim3(dn::grid_for(n, kNT, kGridCap)), dim3(kNT), 0, st, n, d_pos, cig, max_seg, d_n, d_b, d_end);
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(nseg, d_n, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(bounds, d_b, sizeof(int64_t) * (size_t) (n * 2 * max_seg), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(end_pos, d_end, sizeof(int64_t) * (size_t) n, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        return DN_OK;
    });
}

// The annotation and the outputs of one coverage call (the arguments of dn_read_coverage after the reads).
struct CoverageIO {
    int64_t chrom_len, keep_lo, keep_hi;
    int64_t n_exon; const int64_t *exon_iv;
    int64_t n_groups; const int64_t *group_iv; const int32_t *group_gene_off;
    const int32_t *ol_gene; const int64_t *ol_gene_start0, *ol_cov_off; const int32_t *ol_exon_off; const int64_t *ol_exon_bounds;
    int64_t n_iso; const int64_t *iso_iv; const int32_t *iso_gene;
    int64_t n_iso_union; const int64_t *iso_union;
    int64_t n_genes; int64_t *counts, *ol_cov;
    int64_t csr_cap; int64_t *nnz; int32_t *csr_idx; int64_t *csr_val;
    int64_t *n_isolated_reads; double *device_ms;
};

// The coverage stages on n_rows device-resident rows (positions d_pos, CIGARs `cig`), queued on `st` after whatever the
// caller queued there (its uploads).  pair_id (host, paired only) is checked and uploaded here; d_pair_id, when not NULL,
// is the same array already on the device and the library's own (dn_bam_rows_pair): pair_id is then not read.
// mates.flag != NULL (BamCigars with d_pair_id only): the pairs are those of the FLAG rule (MateBits).
// cigar_text(r) gives row r's CIGAR as text for the error messages.
template <class C>
int coverage_stages(hipStream_t st, int32_t paired, int64_t n_rows, const int64_t *d_pos, C cig, const int32_t *pair_id,
                    const int32_t *d_pair_id, int64_t n_pair_ids, const CoverageIO &io, const std::function<std::string(int64_t)> &cigar_text,
                    MateBits mates = MateBits{}, StrandSel sel = StrandSel{})
{
    constexpr bool kCanMate = std::is_same<C, BamCigars>::value;
    if (sel.want != 0 && ((sel.want != dn::kSensePlus && sel.want != dn::kSenseMinus) || (n_rows > 0 && !sel.sense)))
        return dn::fail(DN_E_INVALID, "dn_read_coverage: a stranded call takes the sense of every row and the strand '+' or '-'");
    if (mates.flag && (!kCanMate || !paired || !d_pair_id || !mates.order || n_rows > kMateRowsMax))
        return dn::fail(n_rows > kMateRowsMax ? DN_E_UNSUPPORTED : DN_E_INVALID, "dn_read_coverage: pairing by FLAG takes a paired row store of at most 2^30 rows");
    const int64_t chrom_len = io.chrom_len, n_exon = io.n_exon, n_groups = io.n_groups, n_iso = io.n_iso, n_iso_union = io.n_iso_union,
                  n_genes = io.n_genes, csr_cap = io.csr_cap;
    if (n_rows < 0 || n_rows > INT32_MAX - 1 || chrom_len <= 0 || chrom_len > INT32_MAX - 4 || n_exon < 0 || n_groups < 0 || n_iso < 0 || n_iso_union < 0 ||
        n_genes < 0 || !io.counts || !io.nnz || !io.n_isolated_reads || (paired && n_rows > 0 && ((!pair_id && !d_pair_id) || n_pair_ids < 1)) ||
        (n_groups > 0 && (!io.group_iv || !io.group_gene_off || !io.ol_cov || !io.ol_cov_off)) ||
        (n_iso > 0 && (!io.iso_iv || !io.iso_gene || !io.iso_union)) || csr_cap < 0 || (csr_cap > 0 && (!io.csr_idx || !io.csr_val)))
        return dn::fail(DN_E_INVALID, "dn_read_coverage: bad argument");
    if (paired && !d_pair_id)
        for (int64_t r = 0; r < n_rows; r++)
            if (pair_id[r] < 0 || pair_id[r] >= n_pair_ids) return dn::fail(DN_E_INVALID, "dn_read_coverage: pair id out of range");
    const int32_t *group_gene_off = io.group_gene_off, *ol_gene = io.ol_gene, *ol_exon_off = io.ol_exon_off, *iso_gene = io.iso_gene;
    const int64_t *ol_cov_off = io.ol_cov_off, *exon_iv = io.exon_iv;
    const int64_t n_ol = n_groups > 0 ? group_gene_off[n_groups] : 0;
    const int64_t ol_total = n_ol > 0 ? ol_cov_off[n_ol] : 0;
    // every index the kernels follow stays inside its array
    for (int64_t g = 0; g < n_groups; g++)
        if (group_gene_off[g] < 0 || group_gene_off[g + 1] < group_gene_off[g]) return dn::fail(DN_E_INVALID, "dn_read_coverage: bad group_gene_off");
    for (int64_t q = 0; q < n_ol; q++)
        if (ol_gene[q] < 0 || ol_gene[q] >= n_genes || ol_cov_off[q + 1] - ol_cov_off[q] < 2 || ol_exon_off[q + 1] < ol_exon_off[q] ||
            (q == 0 && (ol_cov_off[0] != 0 || ol_exon_off[0] != 0))) return dn::fail(DN_E_INVALID, "dn_read_coverage: bad overlap-gene tables");
    for (int64_t k = 0; k < n_iso; k++)
        if (iso_gene[k] < 0 || iso_gene[k] >= n_genes) return dn::fail(DN_E_INVALID, "dn_read_coverage: bad iso_gene");
    for (int64_t k = 0; k < n_exon; k++)
        if (exon_iv[2 * k] < 0 || exon_iv[2 * k + 1] >= chrom_len) return dn::fail(DN_E_INVALID, "dn_read_coverage: exon union outside the chromosome");
    const int64_t n_ol_exon = n_ol > 0 ? ol_exon_off[n_ol] : 0;
    dn::DeviceBuffer<int64_t> d_end, d_exon, d_giv, d_gs0, d_coff, d_oex, d_iiv, d_iu;
    dn::DeviceBuffer<int64_t> d_val64, d_csr_val;
    dn::DeviceBuffer<int32_t> d_pid, d_pcnt, d_rank, d_rows, d_keep, d_ggo, d_olg, d_oxo, d_ig, d_csr_idx;
    dn::DeviceBuffer<int> d_counts, d_oldiff, d_olcov, d_cdiff, d_ccov, d_nsel;
    dn::DeviceBuffer<unsigned long long> d_niso, d_err;
    dn::Scratch scratch;                             // of the scans and the select
    dn::Event e0, e1;
    unsigned long long h_err[3], h_niso = 0;         // what the stream copies to the host
    int h_nsel = 0;
    int32_t survivors = 0;
    const int32_t *p_pid = d_pair_id;                // the pair ids the kernels read: the caller's, or the upload in d_pid
    std::vector<int> h_counts(n_genes > 0 ? n_genes : 1);
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(alloc_padded(d_end, n_rows)); DN_TRY(alloc_padded(d_keep, n_rows + 1));
        DN_TRY(alloc_padded(d_exon, 2 * n_exon)); DN_TRY(alloc_padded(d_giv, 2 * n_groups)); DN_TRY(alloc_padded(d_ggo, n_groups + 1));
        DN_TRY(alloc_padded(d_olg, n_ol)); DN_TRY(alloc_padded(d_gs0, n_ol)); DN_TRY(alloc_padded(d_coff, n_ol + 1));
        DN_TRY(alloc_padded(d_oxo, n_ol + 1)); DN_TRY(alloc_padded(d_oex, 2 * n_ol_exon));
        DN_TRY(alloc_padded(d_iiv, 2 * n_iso)); DN_TRY(alloc_padded(d_ig, n_iso)); DN_TRY(alloc_padded(d_iu, 2 * n_iso_union));
        DN_TRY(alloc_padded(d_counts, n_genes)); DN_TRY(alloc_padded(d_oldiff, ol_total)); DN_TRY(alloc_padded(d_olcov, ol_total));
        DN_TRY(alloc_padded(d_val64, ol_total));
        DN_TRY(alloc_padded(d_cdiff, chrom_len + 1)); DN_TRY(alloc_padded(d_ccov, chrom_len + 1));
        DN_TRY(alloc_padded(d_csr_idx, chrom_len)); DN_TRY(alloc_padded(d_csr_val, chrom_len)); DN_TRY(alloc_padded(d_nsel, 1));
        DN_TRY(alloc_padded(d_niso, 1)); DN_TRY(alloc_padded(d_err, 3));
        if (paired) {
            if (!d_pair_id) { DN_TRY(alloc_padded(d_pid, n_rows)); p_pid = d_pid; }
            DN_TRY(alloc_padded(d_pcnt, n_pair_ids)); DN_TRY(alloc_padded(d_rank, n_rows + 1));
            DN_TRY(alloc_padded(d_rows, n_rows));
        }
#define H2D(d, h, n) do { if ((n) > 0) DN_TRY(hipMemcpyAsync(d, h, sizeof(*(d)) * (size_t) (n), hipMemcpyHostToDevice, st)); } while (0)
        H2D(d_exon, exon_iv, 2 * n_exon); H2D(d_giv, io.group_iv, 2 * n_groups); H2D(d_ggo, group_gene_off, n_groups > 0 ? n_groups + 1 : 0);
        H2D(d_olg, ol_gene, n_ol); H2D(d_gs0, io.ol_gene_start0, n_ol); H2D(d_coff, ol_cov_off, n_ol > 0 ? n_ol + 1 : 0);
        H2D(d_oxo, ol_exon_off, n_ol > 0 ? n_ol + 1 : 0); H2D(d_oex, io.ol_exon_bounds, 2 * n_ol_exon);
        H2D(d_iiv, io.iso_iv, 2 * n_iso); H2D(d_ig, iso_gene, n_iso); H2D(d_iu, io.iso_union, 2 * n_iso_union);
        if (paired && !d_pair_id) H2D(d_pid, pair_id, n_rows);
#undef H2D
        DN_TRY(hipEventRecord(e0, st));
        DN_TRY(hipMemsetAsync(d_counts, 0, sizeof(int) * (size_t) (n_genes > 0 ? n_genes : 1), st));
        DN_TRY(hipMemsetAsync(d_oldiff, 0, sizeof(int) * (size_t) (ol_total > 0 ? ol_total : 1), st));
        DN_TRY(hipMemsetAsync(d_cdiff, 0, sizeof(int) * (size_t) (chrom_len + 1), st));
        DN_TRY(hipMemsetAsync(d_niso, 0, sizeof(unsigned long long), st));
        DN_TRY(hipMemsetAsync(d_err, 0xff, 3 * sizeof(unsigned long long), st));
        if (paired) DN_TRY(hipMemsetAsync(d_pcnt, 0, sizeof(int32_t) * (size_t) n_pair_ids, st));
        if (n_rows > 0) {
            const dim3 pre_grid(dn::grid_for(n_rows, kNT, kGridCap));
            const int32_t *pre_pid = mates.flag || paired ? p_pid : nullptr;
            if constexpr (kCanMate) {
                if (mates.flag && sel.want)
                    hipLaunchKernelGGL((k_prefilter<C, true, true, StrandSel>), pre_grid, dim3(kNT), 0, st, n_rows, d_pos, cig, io.keep_lo, io.keep_hi,
                                       pre_pid, d_pcnt.get(), mates, d_end.get(), d_keep.get(), sel);
                else if (mates.flag)
                    hipLaunchKernelGGL((k_prefilter<C, true, false>), pre_grid, dim3(kNT), 0, st, n_rows, d_pos, cig, io.keep_lo, io.keep_hi, pre_pid,
                                       d_pcnt.get(), mates, d_end.get(), d_keep.get());
            }
            if (!mates.flag && sel.want)
                hipLaunchKernelGGL((k_prefilter<C, false, true, StrandSel>), pre_grid, dim3(kNT), 0, st, n_rows, d_pos, cig, io.keep_lo, io.keep_hi,
                                   pre_pid, d_pcnt.get(), mates, d_end.get(), d_keep.get(), sel);
            else if (!mates.flag)
                hipLaunchKernelGGL((k_prefilter<C, false, false>), pre_grid, dim3(kNT), 0, st, n_rows, d_pos, cig, io.keep_lo, io.keep_hi, pre_pid,
                                   d_pcnt.get(), mates, d_end.get(), d_keep.get());
            DN_TRY(hipGetLastError());
            int64_t n_units = n_rows;
            if (paired) {
                hipLaunchKernelGGL(k_pair_flag, dim3(dn::grid_for(n_rows, kNT, kGridCap)), dim3(kNT), 0, st, n_rows, p_pid, d_pcnt.get(),
                                   mates.flag ? kMatePair : 2, d_keep.get());
                DN_TRY(hipGetLastError());
                // exclusive rank of every surviving row; rank[n_rows] is the number of survivors
                DN_TRY(hipMemsetAsync(d_keep + n_rows, 0, sizeof(int32_t), st));       // keep[n_rows] = 0: rank[n_rows] = #survivors
                DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
                    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_keep.get(), d_rank.get(), (int) n_rows + 1, st);
                }));
                hipLaunchKernelGGL(k_pair_compact, dim3(dn::grid_for(n_rows, kNT, kGridCap)), dim3(kNT), 0, st, n_rows, d_keep, d_rank, d_rows);
                DN_TRY(hipGetLastError());
                DN_TRY(hipMemcpyAsync(&survivors, d_rank + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                DN_TRY(hipStreamSynchronize(st));
                n_units = survivors / 2;
            }
            if (n_units > 0) {
                ReadsArgs<C> A;
                A.paired = paired; A.n_units = n_units; A.pos = d_pos; A.end_pos = d_end; A.cig = cig;
                A.keep = d_keep; A.rows = d_rows;
                A.n_exon = n_exon; A.exon_iv = d_exon; A.n_groups = n_groups; A.group_iv = d_giv; A.group_gene_off = d_ggo;
                A.ol_gene = d_olg; A.ol_gstart0 = d_gs0; A.ol_cov_off = d_coff; A.ol_exon_off = d_oxo; A.ol_exon = d_oex;
                A.n_iso = n_iso; A.iso_iv = d_iiv; A.iso_gene = d_ig; A.n_iso_union = n_iso_union; A.iso_union = d_iu;
                A.counts = d_counts; A.ol_diff = d_oldiff; A.chrom_diff = d_cdiff; A.n_iso_reads = d_niso; A.err = d_err;
                hipLaunchKernelGGL(k_reads<C>, dim3(dn::grid_for(n_units, kNT, kGridCap)), dim3(kNT), 0, st, A);
                DN_TRY(hipGetLastError());
            }
        }
        // difference arrays -> coverage
        DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::InclusiveSum(tmp, bytes, d_cdiff.get(), d_ccov.get(), (int) chrom_len, st);
        }));
        if (ol_total > 0) {
            DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
                return hipcub::DeviceScan::InclusiveSum(tmp, bytes, d_oldiff.get(), d_olcov.get(), (int) ol_total, st);
            }));
            hipLaunchKernelGGL(k_widen, dim3(dn::grid_for(ol_total, kNT, kGridCap)), dim3(kNT), 0, st, ol_total, d_olcov, d_val64);
            DN_TRY(hipGetLastError());
        }
        // chromosome vector -> CSR (positions ascending)
        DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceSelect::If(tmp, bytes, hipcub::CountingInputIterator<int32_t>(0), d_csr_idx.get(), d_nsel.get(), (int) chrom_len,
                                            NonZero{d_ccov.get()}, st);
        }));
        DN_TRY(hipMemcpyAsync(&h_nsel, d_nsel, sizeof(int), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(&h_niso, d_niso, sizeof(h_niso), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (h_nsel > 0) {
            hipLaunchKernelGGL(k_gather_csr, dim3(dn::grid_for(h_nsel, kNT, kGridCap)), dim3(kNT), 0, st, (int64_t) h_nsel, d_csr_idx, d_ccov, d_csr_val);
            DN_TRY(hipGetLastError());
        }
        DN_TRY(hipEventRecord(e1, st));
        if (h_err[0] != ~0ull)
            return dn::fail(DN_E_INVALID, "CIGAR string " + cigar_text((int64_t) h_err[0]) + " has no matching region.");
        if (h_err[1] != ~0ull)
            return dn::fail(DN_E_UNSUPPORTED, "CIGAR string " + cigar_text((int64_t) h_err[1]) + " has more than " + std::to_string(kMaxSeg) +
                                              " match segments (DN_READS_MAX_SEG)");
        if (h_err[2] != ~0ull)
            return dn::fail(DN_E_INVALID, "an overlap gene's exons reach past its gene span (row " + std::to_string(h_err[2]) + ")");
        if (h_nsel > csr_cap)
            return dn::fail(DN_E_INVALID, "dn_read_coverage: " + std::to_string(h_nsel) + " nonzeros exceed csr_cap " + std::to_string(csr_cap));
        *io.nnz = h_nsel;
        *io.n_isolated_reads = (int64_t) h_niso;
        if (h_nsel > 0) {
            DN_TRY(hipMemcpyAsync(io.csr_idx, d_csr_idx, sizeof(int32_t) * (size_t) h_nsel, hipMemcpyDeviceToHost, st));
            DN_TRY(hipMemcpyAsync(io.csr_val, d_csr_val, sizeof(int64_t) * (size_t) h_nsel, hipMemcpyDeviceToHost, st));
        }
        if (ol_total > 0) DN_TRY(hipMemcpyAsync(io.ol_cov, d_val64, sizeof(int64_t) * (size_t) ol_total, hipMemcpyDeviceToHost, st));
        if (n_genes > 0) DN_TRY(hipMemcpyAsync(h_counts.data(), d_counts, sizeof(int) * (size_t) n_genes, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        for (int64_t k = 0; k < n_genes; k++) io.counts[k] = h_counts[k];
        if (io.device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *io.device_ms = ms; }
        return DN_OK;
    });
}

}  // namespace

#define COVERAGE_IO                                                                                                    \
    CoverageIO io{chrom_len, keep_lo, keep_hi, n_exon, exon_iv, n_groups, group_iv, group_gene_off, ol_gene, ol_gene_start0, \
                  ol_cov_off, ol_exon_off, ol_exon_bounds, n_iso, iso_iv, iso_gene, n_iso_union, iso_union, n_genes, counts,  \
                  ol_cov, csr_cap, nnz, csr_idx, csr_val, n_isolated_reads, device_ms}

// dn_read_coverage, and with strand != 0 its stranded sibling: `sense` is then uploaded with the rows
static int read_coverage(int device, int32_t paired, int64_t n_rows, const int64_t *pos, const int64_t *cigar_off, const uint8_t *cigar,
                         const int32_t *pair_id, int64_t n_pair_ids, const uint8_t *sense, uint8_t strand, const CoverageIO &io)
{
    if (n_rows < 0 || n_rows > INT32_MAX - 1 || (n_rows > 0 && (!pos || !cigar_off || !cigar)))
        return dn::fail(DN_E_INVALID, "dn_read_coverage: bad argument");
    const int64_t n_bytes = n_rows > 0 ? cigar_off[n_rows] : 0;
    dn::DeviceBuffer<int64_t> d_pos, d_off;
    dn::DeviceBuffer<uint8_t> d_cig, d_sense;
    dn::Stream st;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(alloc_padded(d_pos, n_rows)); DN_TRY(alloc_padded(d_off, n_rows + 1)); DN_TRY(alloc_padded(d_cig, n_bytes));
        if (n_rows > 0) {
            DN_TRY(hipMemcpyAsync(d_pos, pos, sizeof(int64_t) * (size_t) n_rows, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_off, cigar_off, sizeof(int64_t) * (size_t) (n_rows + 1), hipMemcpyHostToDevice, st));
        }
        if (n_bytes > 0) DN_TRY(hipMemcpyAsync(d_cig, cigar, (size_t) n_bytes, hipMemcpyHostToDevice, st));
        StrandSel sel;
        if (strand) {
            DN_TRY(alloc_padded(d_sense, n_rows));
            if (n_rows > 0) DN_TRY(hipMemcpyAsync(d_sense, sense, (size_t) n_rows, hipMemcpyHostToDevice, st));
            sel.sense = d_sense;
            sel.want = strand;
        }
        return coverage_stages(st, paired, n_rows, d_pos, StrCigars{d_off, d_cig}, pair_id, nullptr, n_pair_ids, io, [&](int64_t r) {
            return std::string((const char *) cigar + cigar_off[r], (size_t) (cigar_off[r + 1] - cigar_off[r]));
        }, MateBits{}, sel);
    });
}

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
    dn::clear_error();
    COVERAGE_IO;
    return read_coverage(device, paired, n_rows, pos, cigar_off, cigar, pair_id, n_pair_ids, nullptr, 0, io);
}

// '+' or '-' as the selector of a stranded call; 0 for anything else
static uint8_t strand_selector(int32_t strand) { return strand == dn::kSensePlus || strand == dn::kSenseMinus ? (uint8_t) strand : 0; }

extern "C" int dn_read_coverage_strand(int device, int32_t paired, int64_t n_rows, const int64_t *pos, const int64_t *cigar_off,
                                       const uint8_t *cigar, const int32_t *pair_id, int64_t n_pair_ids, const uint8_t *sense, int32_t strand,
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
    dn::clear_error();
    if (!strand_selector(strand) || (n_rows > 0 && !sense))
        return dn::fail(DN_E_INVALID, "dn_read_coverage_strand: bad argument (the sense of every row, and the strand '+' or '-')");
    for (int64_t r = 0; r < n_rows; r++)
        if (sense[r] != dn::kSensePlus && sense[r] != dn::kSenseMinus)
            return dn::fail(DN_E_INVALID, "dn_read_coverage_strand: the sense of row " + std::to_string(r) + " is neither '+' nor '-'");
    COVERAGE_IO;
    return read_coverage(device, paired, n_rows, pos, cigar_off, cigar, pair_id, n_pair_ids, sense, strand_selector(strand), io);
}

extern "C" int dn_read_sense_host(int64_t n, const uint16_t *flag, const uint8_t *name_last, int32_t by_name, int32_t stranded, uint8_t *sense)
{
    dn::clear_error();
    if (n < 0 || (n > 0 && (!flag || !name_last || !sense)) || (stranded != dn::kStrandForward && stranded != dn::kStrandReverse))
        return dn::fail(DN_E_INVALID, "dn_read_sense_host: bad argument (stranded 1, forward, or 2, reverse)");
    for (int64_t r = 0; r < n; r++) sense[r] = dn::row_sense(flag[r], name_last[r], by_name != 0, stranded);
    return DN_OK;
}

extern "C" int dn_reads_cigar_bounds(int device, int64_t n, const int64_t *pos, const int64_t *cigar_off, const uint8_t *cigar,
                                     int32_t max_seg, int32_t *nseg, int64_t *bounds, int64_t *end_pos)
{
    dn::clear_error();
    if (n < 0 || max_seg < 1 || max_seg > kMaxSeg || (n > 0 && (!pos || !cigar_off || !cigar || !nseg || !bounds || !end_pos)))
        return dn::fail(DN_E_INVALID, "dn_reads_cigar_bounds: bad argument");
    if (n == 0) return DN_OK;
    dn::DeviceBuffer<int64_t> d_off;
    dn::DeviceBuffer<uint8_t> d_cig;
    dn::Stream st;
    const int64_t n_bytes = cigar_off[n];
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(alloc_padded(d_off, n + 1)); DN_TRY(alloc_padded(d_cig, n_bytes));
        DN_TRY(hipMemcpyAsync(d_off, cigar_off, sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice, st));
        if (n_bytes > 0) DN_TRY(hipMemcpyAsync(d_cig, cigar, (size_t) n_bytes, hipMemcpyHostToDevice, st));
        return cigar_debug(st, n, pos, StrCigars{d_off, d_cig}, max_seg, nseg, bounds, end_pos);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// BAM records -> device-resident rows (NativeBamReadsProcessor, degnorm_amd/bam.py).
//
// The host inflates one window of a chromosome's BGZF blocks and frames it (dn_bam_frame: the start of every complete
// record), or the window is framed where it lies on the device (dn_frame.hip; dn_bam_rows_append_framed, and
// dn_bam_rows_inflate_framed, after which a window's inflated bytes never visit the host); k_bam_scan decodes every
// record of the window and applies the reference's read filters (reads.py load_chromosome_reads), three scans give each kept row its place, and k_bam_write appends the kept rows, in file order,
// to the row store: position, binary CIGAR ops, read name and the length of its qname_unpaired prefix.  The coverage
// stages then read the binary CIGARs in place (BamCigars).  The fixed part of a record is read through dn_bam_record.hpp.
// A store made by dn_bam_rows_create_with runs the scan with the read filters (FLAG masks, MAPQ) in front of the other rules
// and, when it pairs by FLAG, keeps the candidate rows of that rule with their FLAG, MAPQ and PNEXT (the rule:
// include/degnorm_amd.h); the store of dn_bam_rows_create runs the kernels without any of it (k_bam_scan<false>,
// k_bam_write<false>).

namespace {

enum { kBamErrMalformed, kBamErrUnsupported, kBamErrNh, kBamErrNoCigar, kBamNErr };

using dn::le16;
using dn::le32;

struct BamRec : dn::BamHead {
    int64_t aux;                        // where the aux fields begin: a byte offset into the window, as name(), cigar(), end()
};

// the fixed part of the record at window offset o; false when the record does not fit its block_size / the window
__device__ bool bam_parse(const uint8_t *w, int64_t n_bytes, int64_t o, BamRec &R)
{
    if (!dn::bam_head(w, n_bytes, o, R) || R.l_name < 1 || R.l_seq < 0) return false;
    R.aux = R.cigar() + 4 * (int64_t) R.n_cig + ((int64_t) R.l_seq + 1) / 2 + R.l_seq;
    return R.aux <= R.end();
}

__device__ __forceinline__ int aux_size(uint8_t t)
{
    switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
    }
}

// Walk the aux fields [q, end): the first NH tag (nh_state 0 absent, 1 integer with value nh, 2 another type) and whether
// a CG tag is present.  False when a field runs past the record or has an unknown type.
__device__ bool bam_aux(const uint8_t *w, int64_t q, int64_t end, int &nh_state, int64_t &nh, bool &cg)
{
    nh_state = 0;
    nh = 0;
    cg = false;
    while (q < end) {
        if (q + 3 > end) return false;
        const uint8_t t0 = w[q], t1 = w[q + 1], ty = w[q + 2];
        q += 3;
        const bool is_nh = t0 == 'N' && t1 == 'H' && nh_state == 0;
        if (t0 == 'C' && t1 == 'G') cg = true;
        const int sz = aux_size(ty);
        if (sz > 0) {
            if (q + sz > end) return false;
            if (is_nh) {
                nh_state = 1;
                switch (ty) {
                case 'c': nh = (int8_t) w[q]; break;
                case 'C': nh = w[q]; break;
                case 's': nh = (int16_t) le16(w + q); break;
                case 'S': nh = le16(w + q); break;
                case 'i': nh = (int32_t) le32(w + q); break;
                case 'I': nh = le32(w + q); break;
                default: nh_state = 2;                      // A, f
                }
            }
            q += sz;
        } else if (ty == 'Z' || ty == 'H') {
            while (q < end && w[q] != 0) q++;
            if (q >= end) return false;
            q++;
            if (is_nh) nh_state = 2;
        } else if (ty == 'B') {
            if (q + 5 > end) return false;
            const int esz = aux_size(w[q]);
            const int64_t cnt = le32(w + q + 1);
            if (esz == 0 || w[q] == 'A') return false;
            q += 5;
            if (cnt * esz > end - q) return false;
            q += cnt * esz;
            if (is_nh) nh_state = 2;
        } else {
            return false;
        }
    }
    return true;
}

struct BamFilter {
    int32_t tid, unique, paired;
    // the options of dn_bam_rows_create_with (all 0: the store of dn_bam_rows_create)
    int32_t by_flag;                    // a paired store whose rows are the candidates of the FLAG rule
    uint32_t exclude, require;
    int32_t min_mapq;
    bool options() const { return by_flag || exclude || require || min_mapq; }
};

enum { kDropFlags, kDropMapq, kDropCandidate, kNDrop };
constexpr int kBamMapq = 13;            // the MAPQ byte of a record

// a record that passed the read filters and the NH rule is a row of a FLAG-rule store
__device__ __forceinline__ bool mate_candidate(const BamRec &R, int32_t tid)
{
    const uint32_t f = R.flag;
    return (f & 0x1u) && !(f & 0xCu) && R.next_ref == tid && ((f & dn::kFlagFirst) != 0) != ((f & dn::kFlagLast) != 0);
}

// per record: kept (refID == tid, NH rule, mate rule), its op count and name length when kept; errors (first record index).
// OPTIONS (F.options()): the read filters come first among the rules that drop a well-formed record, the FLAG rule's
// candidate test stands in for the mate rule, and dropped[] counts what each took.
template <bool OPTIONS>
__global__ __launch_bounds__(kNT) void k_bam_scan(const uint8_t *__restrict__ w, int64_t n_bytes, const int64_t *__restrict__ rec_off,
                                                  int64_t n_rec, BamFilter F, int32_t *__restrict__ keep, int32_t *__restrict__ n_ops,
                                                  int32_t *__restrict__ n_name, unsigned long long *__restrict__ err,
                                                  unsigned long long *__restrict__ dropped)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n_rec; i += (int64_t) gridDim.x * kNT) {
        BamRec R;
        int32_t k = 0;
        if (!bam_parse(w, n_bytes, rec_off[i], R)) {
            atomicMin(err + kBamErrMalformed, (unsigned long long) i);
        } else if (R.ref == F.tid) {
            int nh_state;
            int64_t nh;
            bool cg;
            k = 1;
            if (!bam_aux(w, R.aux, R.end(), nh_state, nh, cg)) { atomicMin(err + kBamErrMalformed, (unsigned long long) i); k = 0; }
            else if (OPTIONS && ((R.flag & F.exclude) != 0 || (R.flag & F.require) != F.require)) { atomicAdd(dropped + kDropFlags, 1ull); k = 0; }
            else if (OPTIONS && (int32_t) w[R.o + kBamMapq] < F.min_mapq) { atomicAdd(dropped + kDropMapq, 1ull); k = 0; }
            else if (F.unique && nh_state == 2) { atomicMin(err + kBamErrNh, (unsigned long long) i); k = 0; }
            else if (F.unique && nh_state == 1 && nh > 1) k = 0;
            else if (OPTIONS && F.by_flag) { if (!mate_candidate(R, F.tid)) { atomicAdd(dropped + kDropCandidate, 1ull); k = 0; } }
            else if (F.paired && R.next_ref == -1) k = 0;
            if (k) {
                if (R.n_cig == 0) atomicMin(err + kBamErrNoCigar, (unsigned long long) i);
                bool bad = false;
                for (uint32_t c = 0; c < R.n_cig; c++) bad |= (le32(w + R.cigar() + 4 * (int64_t) c) & 15u) > 8u;
                // a CIGAR moved to the CG tag leaves <l_seq>S<ref_len>N in the record
                if (cg && R.n_cig == 2 && le32(w + R.cigar()) == (((uint32_t) R.l_seq << 4) | 4u) && (le32(w + R.cigar() + 4) & 15u) == 3u)
                    bad = true;
                if (bad) atomicMin(err + kBamErrUnsupported, (unsigned long long) i);
            }
        }
        keep[i] = k;
        n_ops[i] = k ? (int32_t) R.n_cig : 0;
        n_name[i] = k ? (int32_t) R.l_name - 1 : 0;
    }
}

struct BamRowsOut {
    int64_t *pos, *op_beg, *name_beg;
    int32_t *n_op, *name_len, *key_len;
    uint32_t *ops;
    uint8_t *names;
    int32_t *max_key;
    // a FLAG-rule store only
    uint16_t *flag;
    uint8_t *mapq;
    int32_t *next_pos;
};

// MATES: the rows of a FLAG-rule store, which keep FLAG, MAPQ and PNEXT and whose key is the whole name
template <bool MATES>
__global__ __launch_bounds__(kNT) void k_bam_write(const uint8_t *__restrict__ w, int64_t n_bytes, const int64_t *__restrict__ rec_off,
                                                   int64_t n_rec, const int32_t *__restrict__ keep, const int32_t *__restrict__ rank,
                                                   const int32_t *__restrict__ op_rank, const int32_t *__restrict__ name_rank,
                                                   int64_t row0, int64_t op0, int64_t name0, BamRowsOut O)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n_rec; i += (int64_t) gridDim.x * kNT) {
        BamRec R;
        if (!keep[i] || !bam_parse(w, n_bytes, rec_off[i], R)) continue;
        const int64_t r = row0 + rank[i], ob = op0 + op_rank[i], nb = name0 + name_rank[i];
        const int32_t nl = (int32_t) R.l_name - 1;
        O.pos[r] = R.pos;
        O.op_beg[r] = ob;
        O.n_op[r] = (int32_t) R.n_cig;
        for (uint32_t c = 0; c < R.n_cig; c++) O.ops[ob + c] = le32(w + R.cigar() + 4 * (int64_t) c);
        int32_t key = 0;                        // qname_unpaired = the name up to its last '.', '' without one
        for (int32_t c = 0; c < nl; c++) {
            const uint8_t ch = w[R.name() + c];
            O.names[nb + c] = ch;
            if (ch == '.') key = c;
        }
        if (MATES) {
            key = nl;
            O.flag[r] = (uint16_t) R.flag;
            O.mapq[r] = w[R.o + kBamMapq];
            O.next_pos[r] = R.next_pos;
        }
        O.name_beg[r] = nb;
        O.name_len[r] = nl;
        O.key_len[r] = key;
        atomicMax(O.max_key, key);
    }
}

// A stranded store (dn_bam_rows_set_stranded): the sense of every kept record of the window (dn::row_sense), written to the
// row k_bam_write gave it.  One lane per record, while the window is resident; by_name: a paired store of the name rule.
__global__ __launch_bounds__(kNT) void k_bam_sense(const uint8_t *__restrict__ w, int64_t n_bytes, const int64_t *__restrict__ rec_off,
                                                   int64_t n_rec, const int32_t *__restrict__ keep, const int32_t *__restrict__ rank,
                                                   int64_t row0, int32_t by_name, int32_t protocol, uint8_t *__restrict__ sense)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n_rec; i += (int64_t) gridDim.x * kNT) {
        BamRec R;
        if (!keep[i] || !bam_parse(w, n_bytes, rec_off[i], R)) continue;
        const uint8_t name_last = R.l_name > 1 ? w[R.name() + R.l_name - 2] : 0;      // l_name counts the NUL
        sense[row0 + rank[i]] = dn::row_sense(R.flag, name_last, by_name != 0, protocol);
    }
}

__global__ __launch_bounds__(kNT) void k_bam_keys(int64_t n, const int64_t *__restrict__ name_beg, const int32_t *__restrict__ key_len,
                                                  const uint8_t *__restrict__ names, int32_t width, uint8_t *__restrict__ out)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT)
        for (int32_t c = 0; c < width; c++) out[r * width + c] = c < key_len[r] ? names[name_beg[r] + c] : 0;
}

__global__ __launch_bounds__(kNT) void k_bam_gather(int64_t n, const int32_t *__restrict__ order, const int64_t *__restrict__ pos,
                                                    const int64_t *__restrict__ op_beg, const int32_t *__restrict__ n_op,
                                                    int64_t *__restrict__ pos_o, int64_t *__restrict__ op_beg_o, int32_t *__restrict__ n_op_o)
{
    for (int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t) gridDim.x * kNT) {
        const int32_t s = order[r];
        pos_o[r] = pos[s]; op_beg_o[r] = op_beg[s]; n_op_o[r] = n_op[s];
    }
}

std::string bam_name(const uint8_t *w, int64_t n_bytes, int64_t o)
{
    if (o + dn::kBamName > n_bytes) return "?";
    const int64_t l = w[o + dn::kBamLName];
    if (l < 1 || o + dn::kBamName + l > n_bytes) return "?";
    return std::string((const char *) w + o + dn::kBamName, (size_t) (l - 1));
}

std::string cigar_string(const uint32_t *ops, int64_t n)
{
    std::string s;
    for (int64_t k = 0; k < n; k++) s += std::to_string(ops[k] >> 4) + "MIDNSHP=X"[(ops[k] & 15u) < 9u ? (ops[k] & 15u) : 0];
    return s;
}

}  // namespace

struct dn_bam_rows_s {
    int device;
    BamFilter F;
    dn::Stream st;
    int64_t n_rows = 0, n_ops = 0, n_names = 0;
    dn::GrowBuffer<int64_t> pos, op_beg, name_beg, rec_off;
    dn::GrowBuffer<int32_t> n_op, name_len, key_len;
    dn::DeviceBuffer<int32_t> max_key;
    // a FLAG-rule store's FLAG, MAPQ and PNEXT per row, and for every store with options what each rule dropped so far
    dn::GrowBuffer<uint16_t> flag;
    dn::GrowBuffer<uint8_t> mapq;
    dn::GrowBuffer<int32_t> next_pos;
    dn::DeviceBuffer<unsigned long long> dropped;
    // strand-specific counting (dn_bam_rows_set_stranded): the protocol, dn::kStrandNo for none, and the sense of every row
    int32_t stranded = dn::kStrandNo;
    dn::GrowBuffer<uint8_t> sense;
    dn::GrowBuffer<int32_t> keep, w_ops, w_name, rank, op_rank, name_rank;
    dn::GrowBuffer<uint32_t> ops;
    dn::GrowBuffer<uint8_t> names, win;
    dn::DeviceBuffer<unsigned long long> err;
    dn::Scratch scratch;                   // of the three scans of a window
    // device inflate (dn_bam_rows_inflate, dn_bam_rows_inflate_framed; armed by dn_bam_rows_expect_crc): the window ingest, the
    // pinned host copy of the window, and the bytes of h->win that hold the resident window (-1: none)
    dn::InflateWindow ingest;
    dn::PinnedBuffer<uint8_t> host_win;
    int64_t cap_host = 0, resident = -1;
    // device framing (dn_bam_rows_append_framed, dn_bam_rows_inflate_framed): its work buffers, the record cut by the end of
    // the window before (dn_bam_rows_inflate_framed keeps it on the device), the segment size asked for (0: the default), the
    // sums dn_bam_rows_frame_info reports and the pos of the last record framed
    dn::FrameWork frame;
    dn::DeviceCarry carry;
    int64_t frame_segment = 0, frame_segments = 0, frame_fixups = 0;
    double frame_ms = 0.0, framed_decode_ms = 0.0;
    int32_t last_pos = INT32_MIN;
    // dn_bam_rows_pair: the rows in qname_unpaired order and the pair id of each row of that order, for the n_rows there
    // were then (has_pairing; an append of rows ends it), and the number of ids
    dn::DeviceBuffer<int32_t> pair_order, pair_id;
    int64_t n_pair_ids = 0;
    bool has_pairing = false;
    std::string no_cigar;                  // the name of the first kept row without CIGAR ops ("" while there is none)
    bool has_no_cigar = false;
};

extern "C" int dn_bam_frame(const uint8_t *buf, int64_t n_bytes, int32_t tid, int32_t *last_pos, int64_t *rec_off, int64_t cap,
                            int64_t *n_rec, int64_t *consumed)
{
    dn::clear_error();
    if (n_bytes < 0 || (n_bytes > 0 && !buf) || cap < 0 || (cap > 0 && !rec_off) || !n_rec || !consumed || (tid >= 0 && !last_pos))
        return dn::fail(DN_E_INVALID, "dn_bam_frame: bad argument");
    int64_t o = 0, n = 0;
    while (o + 4 <= n_bytes) {
        const int32_t bs = (int32_t) dn::le32(buf + o);
        if (bs < dn::kBamMinSize)
            return dn::fail(DN_E_INVALID, "malformed BAM record at byte " + std::to_string(o) + " of the window (block_size " + std::to_string(bs) + ")");
        if (o + 4 + (int64_t) bs > n_bytes) break;          // the tail: carried over to the next window
        if (n >= cap) return dn::fail(DN_E_INVALID, "dn_bam_frame: more records than cap");
        if (tid >= 0) {
            const int32_t ref = (int32_t) dn::le32(buf + o + dn::kBamRef), pos = (int32_t) dn::le32(buf + o + dn::kBamPos);
            if (ref != tid || pos < *last_pos)
                return dn::fail(DN_E_INVALID, "BAM file is not sorted by coordinate, or its index is stale: a record of refID " + std::to_string(ref) +
                                              " at position " + std::to_string(pos) + " follows position " + std::to_string(*last_pos) +
                                              " inside the index range of refID " + std::to_string(tid));
            *last_pos = pos;
        }
        rec_off[n++] = o;
        o += 4 + (int64_t) bs;
    }
    *n_rec = n;
    *consumed = o;
    return DN_OK;
}

static int rows_create(const char *who, int device, const BamFilter &F, dn_bam_rows *out)
{
    *out = nullptr;
    auto h = std::make_unique<dn_bam_rows_s>();
    h->device = device;
    h->F = F;
    DN_TRY_AS(who, hipSetDevice(device));
    DN_TRY_AS(who, h->st.create(hipStreamCreate));
    const int rc = dn::synced(h->st, [&]() -> int {
        DN_TRY_AS(who, alloc_padded(h->max_key, 1));
        DN_TRY_AS(who, alloc_padded(h->err, kBamNErr));
        DN_TRY_AS(who, alloc_padded(h->dropped, kNDrop));
        DN_TRY_AS(who, hipMemsetAsync(h->max_key, 0, sizeof(int32_t), h->st));
        DN_TRY_AS(who, hipMemsetAsync(h->dropped, 0, sizeof(unsigned long long) * kNDrop, h->st));
        DN_TRY_AS(who, hipStreamSynchronize(h->st));
        return DN_OK;
    });
    if (rc == DN_OK) *out = h.release();
    return rc;
}

extern "C" int dn_bam_rows_create(int device, int32_t tid, int32_t unique_alignment, int32_t paired, dn_bam_rows *out)
{
    dn::clear_error();
    if (!out) return dn::fail(DN_E_INVALID, "dn_bam_rows_create: bad argument");
    return rows_create("dn_bam_rows_create", device, BamFilter{tid, unique_alignment ? 1 : 0, paired ? 1 : 0, 0, 0u, 0u, 0}, out);
}

extern "C" int dn_bam_rows_create_with(int device, int32_t tid, int32_t unique_alignment, int32_t paired, const dn_bam_rows_options *opt,
                                       dn_bam_rows *out)
{
    dn::clear_error();
    if (!out || !opt || (opt->pairing != DN_PAIR_BY_NAME && opt->pairing != DN_PAIR_BY_FLAG) || opt->exclude_flags > 0xffffu ||
        opt->require_flags > 0xffffu || opt->min_mapq < 0 || opt->min_mapq > 255)
        return dn::fail(DN_E_INVALID, "dn_bam_rows_create_with: bad argument (pairing 0 or 1, flag masks up to 0xffff, min_mapq 0 .. 255)");
    const int32_t by_flag = paired && opt->pairing == DN_PAIR_BY_FLAG;
    return rows_create("dn_bam_rows_create_with", device,
                       BamFilter{tid, unique_alignment ? 1 : 0, paired ? 1 : 0, by_flag, opt->exclude_flags, opt->require_flags, opt->min_mapq}, out);
}

extern "C" int dn_bam_rows_dropped(dn_bam_rows h, int64_t *by_flags, int64_t *by_mapq, int64_t *not_candidate)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_rows_dropped: bad argument");
    unsigned long long d[kNDrop] = {0, 0, 0};
    DN_TRY(hipSetDevice(h->device));
    const int rc = dn::synced(h->st, [&]() -> int {
        DN_TRY(hipMemcpyAsync(d, h->dropped, sizeof(d), hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    });
    if (rc != DN_OK) return rc;
    if (by_flags) *by_flags = (int64_t) d[kDropFlags];
    if (by_mapq) *by_mapq = (int64_t) d[kDropMapq];
    if (not_candidate) *not_candidate = (int64_t) d[kDropCandidate];
    return DN_OK;
}

extern "C" int dn_bam_rows_fetch_mates(dn_bam_rows h, uint16_t *flag, uint8_t *mapq, int32_t *next_pos)
{
    dn::clear_error();
    if (!h || !h->F.by_flag) return dn::fail(DN_E_INVALID, "dn_bam_rows_fetch_mates: bad argument (a store that pairs by FLAG)");
    hipStream_t st = h->st;
    const size_t n = (size_t) h->n_rows;
    if (n == 0) return DN_OK;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(st, [&]() -> int {
        if (flag) DN_TRY(hipMemcpyAsync(flag, h->flag, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, st));
        if (mapq) DN_TRY(hipMemcpyAsync(mapq, h->mapq, n, hipMemcpyDeviceToHost, st));
        if (next_pos) DN_TRY(hipMemcpyAsync(next_pos, h->next_pos, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        return DN_OK;
    });
}

extern "C" void dn_bam_rows_destroy(dn_bam_rows h)
{
    if (!h) return;
    (void) hipSetDevice(h->device);
    if (h->st) (void) hipStreamSynchronize(h->st);
    delete h;
}

namespace {

// the record offsets of a window framed on the host, to where append_window reads them
int upload_offsets(dn_bam_rows h, const int64_t *rec_off, int64_t n_rec)
{
    DN_TRY(h->rec_off.reserve(n_rec + 1, 0, h->st));
    DN_TRY(hipMemcpyAsync(h->rec_off, rec_off, sizeof(int64_t) * (size_t) n_rec, hipMemcpyHostToDevice, h->st));
    return DN_OK;
}

// Decode, filter and compact the n_rec records of the window in h->win (n_bytes of it), whose offsets are in h->rec_off, and
// append the kept rows.  `window` is a host copy of the same bytes, read only to name a read in an error text; without one
// (NULL) the at most 36 + 255 bytes of that record come from the device.
int append_window(dn_bam_rows h, const uint8_t *window, int64_t n_bytes, int64_t n_rec)
{
    hipStream_t st = h->st;
    int32_t tot[3];                                  // what the stream copies to the host
    unsigned long long herr[kBamNErr];
    int64_t name_off = 0;
    uint8_t name_rec[36 + 255];
    const auto name_of = [&](unsigned long long i) -> std::string {
        if (hipMemcpyAsync(&name_off, h->rec_off + i, sizeof(name_off), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess || name_off < 0 || name_off > n_bytes)
            return "?";
        if (window) return bam_name(window, n_bytes, name_off);
        const int64_t len = n_bytes - name_off < (int64_t) sizeof(name_rec) ? n_bytes - name_off : (int64_t) sizeof(name_rec);
        if (len <= 0 || hipMemcpyAsync(name_rec, h->win + name_off, (size_t) len, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return "?";
        return bam_name(name_rec, len, 0);
    };
    return dn::synced(st, [&]() -> int {
        // per record, and one more for the totals of the scans
        DN_TRY(h->keep.reserve(n_rec + 1, 0, st)); DN_TRY(h->w_ops.reserve(n_rec + 1, 0, st));
        DN_TRY(h->w_name.reserve(n_rec + 1, 0, st)); DN_TRY(h->rank.reserve(n_rec + 1, 0, st)); DN_TRY(h->op_rank.reserve(n_rec + 1, 0, st));
        DN_TRY(h->name_rank.reserve(n_rec + 1, 0, st));
        DN_TRY(hipMemsetAsync(h->err, 0xff, sizeof(unsigned long long) * kBamNErr, st));
        DN_TRY(hipMemsetAsync(h->keep + n_rec, 0, sizeof(int32_t), st));
        DN_TRY(hipMemsetAsync(h->w_ops + n_rec, 0, sizeof(int32_t), st));
        DN_TRY(hipMemsetAsync(h->w_name + n_rec, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(h->F.options() ? k_bam_scan<true> : k_bam_scan<false>, dim3(dn::grid_for(n_rec, kNT, kGridCap)), dim3(kNT), 0, st,
                           (const uint8_t *) h->win.get(), n_bytes, (const int64_t *) h->rec_off.get(), n_rec, h->F, h->keep.get(), h->w_ops.get(),
                           h->w_name.get(), h->err.get(), h->dropped.get());
        DN_TRY(hipGetLastError());
        const auto rank_of = [&](int32_t *flag, int32_t *rank) {      // exclusive; rank[n_rec] is the total
            return h->scratch.run([&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, flag, rank, (int) n_rec + 1, st); });
        };
        DN_TRY(rank_of(h->keep, h->rank)); DN_TRY(rank_of(h->w_ops, h->op_rank)); DN_TRY(rank_of(h->w_name, h->name_rank));
        DN_TRY(hipMemcpyAsync(tot + 0, h->rank + n_rec, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(tot + 1, h->op_rank + n_rec, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(tot + 2, h->name_rank + n_rec, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(herr, h->err, sizeof(herr), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (herr[kBamErrMalformed] != ~0ull)
            return dn::fail(DN_E_INVALID, "malformed BAM record (read " + name_of(herr[kBamErrMalformed]) + ")");
        if (herr[kBamErrNh] != ~0ull)
            return dn::fail(DN_E_INVALID, "read " + name_of(herr[kBamErrNh]) + " has an NH tag of a non-integer type");
        if (herr[kBamErrUnsupported] != ~0ull)
            return dn::fail(DN_E_UNSUPPORTED, "read " + name_of(herr[kBamErrUnsupported]) +
                                              " has a CIGAR op code above 8 or a CIGAR moved to the CG tag (not supported)");
        if (herr[kBamErrNoCigar] != ~0ull && !h->has_no_cigar) {
            h->has_no_cigar = true;
            h->no_cigar = name_of(herr[kBamErrNoCigar]);
        }
        if (h->n_rows + tot[0] > INT32_MAX - 1) return dn::fail(DN_E_UNSUPPORTED, "dn_bam_rows_append: more than 2^31 - 2 rows");
        if (tot[0] > 0) {
            const int64_t n = h->n_rows, rows = n + tot[0];
            DN_TRY(h->pos.reserve(rows, n, st)); DN_TRY(h->op_beg.reserve(rows, n, st)); DN_TRY(h->name_beg.reserve(rows, n, st));
            DN_TRY(h->n_op.reserve(rows, n, st)); DN_TRY(h->name_len.reserve(rows, n, st)); DN_TRY(h->key_len.reserve(rows, n, st));
            DN_TRY(h->ops.reserve(h->n_ops + tot[1], h->n_ops, st));
            DN_TRY(h->names.reserve(h->n_names + tot[2], h->n_names, st));
            if (h->F.by_flag) {
                DN_TRY(h->flag.reserve(rows, n, st)); DN_TRY(h->mapq.reserve(rows, n, st)); DN_TRY(h->next_pos.reserve(rows, n, st));
            }
            BamRowsOut O{h->pos, h->op_beg, h->name_beg, h->n_op, h->name_len, h->key_len, h->ops, h->names, h->max_key, h->flag, h->mapq, h->next_pos};
            hipLaunchKernelGGL(h->F.by_flag ? k_bam_write<true> : k_bam_write<false>, dim3(dn::grid_for(n_rec, kNT, kGridCap)), dim3(kNT), 0, st,
                               (const uint8_t *) h->win.get(), n_bytes, (const int64_t *) h->rec_off.get(), n_rec, (const int32_t *) h->keep.get(),
                               (const int32_t *) h->rank.get(), (const int32_t *) h->op_rank.get(), (const int32_t *) h->name_rank.get(), h->n_rows,
                               h->n_ops, h->n_names, O);
            DN_TRY(hipGetLastError());
            if (h->stranded != dn::kStrandNo) {
                DN_TRY(h->sense.reserve(rows, n, st));
                hipLaunchKernelGGL(k_bam_sense, dim3(dn::grid_for(n_rec, kNT, kGridCap)), dim3(kNT), 0, st, (const uint8_t *) h->win.get(), n_bytes,
                                   (const int64_t *) h->rec_off.get(), n_rec, (const int32_t *) h->keep.get(), (const int32_t *) h->rank.get(), h->n_rows,
                                   (int32_t) (h->F.paired && !h->F.by_flag), h->stranded, h->sense.get());
                DN_TRY(hipGetLastError());
            }
            DN_TRY(hipStreamSynchronize(st));
            h->n_rows += tot[0];
            h->has_pairing = false;
            h->n_ops += tot[1];
            h->n_names += tot[2];
        }
        return DN_OK;
    });
}

int check_offsets(const char *who, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec)
{
    for (int64_t i = 0; i < n_rec; i++)              // the kernels read 36 bytes at every offset: keep them inside the window
        if (rec_off[i] < 0 || rec_off[i] + 36 > n_bytes) return dn::fail(DN_E_INVALID, std::string(who) + ": record offset outside the window");
    return DN_OK;
}

}  // namespace

extern "C" int dn_bam_rows_append(dn_bam_rows h, const uint8_t *window, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec)
{
    dn::clear_error();
    if (!h || n_bytes < 0 || n_bytes > INT32_MAX || n_rec < 0 || (n_rec > 0 && (!window || !rec_off)))
        return dn::fail(DN_E_INVALID, "dn_bam_rows_append: bad argument");
    if (n_rec == 0) return DN_OK;
    const int rc = check_offsets("dn_bam_rows_append", n_bytes, rec_off, n_rec);
    if (rc != DN_OK) return rc;
    DN_TRY(hipSetDevice(h->device));
    h->resident = -1;
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(h->win.reserve(n_bytes, 0, h->st));         // window scratch: nothing to keep (the previous append has finished)
        DN_TRY(hipMemcpyAsync(h->win, window, (size_t) n_bytes, hipMemcpyHostToDevice, h->st));
        const int urc = upload_offsets(h, rec_off, n_rec);
        return urc != DN_OK ? urc : append_window(h, window, n_bytes, n_rec);
    });
}

// plan the window of an inflate call of the store behind `base` carried bytes
static int plan_window(dn_bam_rows h, const char *who, int64_t base, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                       const int32_t *pay_len, const int32_t *isize, int32_t head_skip, int32_t tail_keep, int64_t &total)
{
    const int rc = h->ingest.plan(who, "dn_bam_rows_expect_crc", n_comp, n_blocks, pay_off, pay_len, isize, head_skip, tail_keep, base, total);
    if (rc != DN_OK) return rc;
    return total > INT32_MAX ? dn::window_size_error(who) : DN_OK;
}

extern "C" int dn_bam_rows_expect_crc(dn_bam_rows h, const uint32_t *crc32, int64_t n_blocks)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_rows_expect_crc: bad argument");
    return h->ingest.arm("dn_bam_rows_expect_crc", crc32, n_blocks);
}

extern "C" int dn_bam_rows_inflate(dn_bam_rows h, const uint8_t *carry, int64_t n_carry, const uint8_t *comp, int64_t n_comp,
                                   int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len, const int32_t *isize,
                                   int32_t head_skip, int32_t tail_keep, const uint8_t **host_window, int64_t *n_bytes,
                                   int32_t *status, double *device_ms)
{
    dn::clear_error();
    if (h) h->ingest.take();
    if (!h || n_carry < 0 || (n_carry > 0 && !carry) || n_comp < 0 || (n_comp > 0 && !comp) || n_blocks < 0 || n_blocks > INT32_MAX ||
        (n_blocks > 0 && (!pay_off || !pay_len || !isize || !status)) || head_skip < 0 || !host_window || !n_bytes)
        return dn::fail(DN_E_INVALID, "dn_bam_rows_inflate: bad argument");
    int64_t total = 0;
    const int brc = plan_window(h, "dn_bam_rows_inflate", n_carry, n_comp, n_blocks, pay_off, pay_len, isize, head_skip, tail_keep, total);
    if (brc != DN_OK) return brc;
    hipStream_t st = h->st;
    DN_TRY(hipSetDevice(h->device));
    h->resident = -1;
    return dn::synced(st, [&]() -> int {
        DN_TRY(h->win.reserve(total, 0, st));
        if (total + 16 > h->cap_host) {
            const int64_t c = dn::grown_capacity(h->cap_host, total + 16);
            dn::PinnedBuffer<uint8_t> nb;                   // the old copy stays until the new one exists, as in GrowBuffer
            DN_TRY(nb.alloc((size_t) c));
            h->host_win = std::move(nb);
            h->cap_host = c;
        }
        if (n_carry > 0) DN_TRY(hipMemcpyAsync(h->win, carry, (size_t) n_carry, hipMemcpyHostToDevice, st));
        bool ok = true;
        int rc = h->ingest.queue(st, comp, n_comp, h->win, status);
        if (rc != DN_OK) return rc;
        if (total > 0) DN_TRY(hipMemcpyAsync(h->host_win, h->win, (size_t) total, hipMemcpyDeviceToHost, st));
        if ((rc = h->ingest.wait(st, status, device_ms, ok)) != DN_OK) return rc;
        *host_window = h->host_win;
        *n_bytes = total;
        h->resident = ok ? total : -1;
        return DN_OK;
    });
}

extern "C" int dn_bam_rows_append_resident(dn_bam_rows h, const int64_t *rec_off, int64_t n_rec)
{
    dn::clear_error();
    if (!h || n_rec < 0 || (n_rec > 0 && !rec_off)) return dn::fail(DN_E_INVALID, "dn_bam_rows_append_resident: bad argument");
    if (h->resident < 0) return dn::fail(DN_E_STATE, "dn_bam_rows_append_resident: no resident window (dn_bam_rows_inflate first)");
    if (n_rec == 0) return DN_OK;
    const int rc = check_offsets("dn_bam_rows_append_resident", h->resident, rec_off, n_rec);
    if (rc != DN_OK) return rc;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->st, [&]() -> int {
        const int urc = upload_offsets(h, rec_off, n_rec);
        return urc != DN_OK ? urc : append_window(h, h->host_win, h->resident, n_rec);
    });
}

// what every device framing of a store adds to the sums of dn_bam_rows_frame_info
static void count_framing(dn_bam_rows h, const dn::FrameResult &R)
{
    h->frame_segments += R.n_segments;
    h->frame_fixups += R.n_fixups;
    h->frame_ms += R.device_ms;
}

extern "C" int dn_bam_rows_frame_segment(dn_bam_rows h, int64_t segment_bytes)
{
    dn::clear_error();
    if (!h || (segment_bytes != 0 && segment_bytes < dn::kFrameSegmentMin))
        return dn::fail(DN_E_INVALID, "dn_bam_rows_frame_segment: bad argument (segment_bytes is 0 or at least 64)");
    h->frame_segment = segment_bytes;
    return DN_OK;
}

// append_window on a window framed on the device, its host time added to the store's sum
static int append_framed_window(dn_bam_rows h, const uint8_t *window, int64_t n_bytes, int64_t n_rec)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = n_rec > 0 ? append_window(h, window, n_bytes, n_rec) : DN_OK;
    h->framed_decode_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int dn_bam_rows_frame_info(dn_bam_rows h, int64_t *n_segments, int64_t *n_fixups, double *device_ms, double *decode_ms)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_rows_frame_info: bad argument");
    if (n_segments) *n_segments = h->frame_segments;
    if (n_fixups) *n_fixups = h->frame_fixups;
    if (device_ms) *device_ms = h->frame_ms;
    if (decode_ms) *decode_ms = h->framed_decode_ms;
    return DN_OK;
}

extern "C" int dn_bam_rows_append_framed(dn_bam_rows h, const uint8_t *window, int64_t n_bytes, int64_t *consumed)
{
    dn::clear_error();
    if (!h || n_bytes < 0 || n_bytes > INT32_MAX || (n_bytes > 0 && !window) || !consumed)
        return dn::fail(DN_E_INVALID, "dn_bam_rows_append_framed: bad argument");
    dn::FrameResult R;
    DN_TRY(hipSetDevice(h->device));
    h->resident = -1;
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(h->win.reserve(n_bytes, 0, h->st));
        if (n_bytes > 0) DN_TRY(hipMemcpyAsync(h->win, window, (size_t) n_bytes, hipMemcpyHostToDevice, h->st));
        const int rc = dn::frame_window(h->st, h->frame, h->win, n_bytes, h->F.tid, &h->last_pos, h->frame_segment, -1, h->rec_off, R);
        count_framing(h, R);
        if (rc != DN_OK) return rc;
        *consumed = R.consumed;
        return append_framed_window(h, window, n_bytes, R.n_rec);
    });
}

extern "C" int dn_bam_rows_inflate_framed(dn_bam_rows h, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                                          const int32_t *pay_len, const int32_t *isize, int32_t head_skip, int32_t tail_keep,
                                          int32_t *status, int64_t *n_bytes, int64_t *n_carry, double *inflate_ms, double *frame_ms)
{
    dn::clear_error();
    if (h) h->ingest.take();
    if (!h || n_comp < 0 || (n_comp > 0 && !comp) || n_blocks < 0 || n_blocks > INT32_MAX ||
        (n_blocks > 0 && (!pay_off || !pay_len || !isize || !status)) || head_skip < 0 || !n_bytes || !n_carry)
        return dn::fail(DN_E_INVALID, "dn_bam_rows_inflate_framed: bad argument");
    int64_t total = 0;
    const int brc = plan_window(h, "dn_bam_rows_inflate_framed", h->carry.n, n_comp, n_blocks, pay_off, pay_len, isize, head_skip, tail_keep, total);
    if (brc != DN_OK) return brc;
    hipStream_t st = h->st;
    dn::FrameResult R;
    DN_TRY(hipSetDevice(h->device));
    h->resident = -1;
    if (frame_ms) *frame_ms = 0.0;
    return dn::synced(st, [&]() -> int {
        DN_TRY(h->win.reserve(total, 0, st));
        DN_TRY(h->carry.put(st, h->win));                   // the record cut by the end of the window before goes first
        bool ok = true;
        int rc = h->ingest.run(st, comp, n_comp, h->win, status, inflate_ms, ok);
        if (rc != DN_OK) return rc;
        *n_bytes = total;
        *n_carry = h->carry.n;
        if (!ok) return DN_OK;
        rc = dn::frame_window(st, h->frame, h->win, total, h->F.tid, &h->last_pos, h->frame_segment, -1, h->rec_off, R);
        count_framing(h, R);
        if (frame_ms) *frame_ms = R.device_ms;
        if (rc != DN_OK) return rc;
        DN_TRY(h->carry.keep(st, h->win, R.consumed, total));
        *n_carry = h->carry.n;
        return append_framed_window(h, nullptr, total, R.n_rec);
    });
}

extern "C" int dn_bam_rows_info(dn_bam_rows h, int64_t *n_rows, int64_t *n_ops, int64_t *n_name_bytes, int32_t *max_key_len)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_rows_info: bad argument");
    if (n_rows) *n_rows = h->n_rows;
    if (n_ops) *n_ops = h->n_ops;
    if (n_name_bytes) *n_name_bytes = h->n_names;
    if (!max_key_len) return DN_OK;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(hipMemcpyAsync(max_key_len, h->max_key, sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    });
}

extern "C" int dn_bam_rows_keys(dn_bam_rows h, int32_t width, uint8_t *keys)
{
    dn::clear_error();
    if (!h || width < 1 || (h->n_rows > 0 && !keys)) return dn::fail(DN_E_INVALID, "dn_bam_rows_keys: bad argument");
    if (h->n_rows == 0) return DN_OK;
    int32_t mk = 0;
    dn::DeviceBuffer<uint8_t> d_keys;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(hipMemcpyAsync(&mk, h->max_key, sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        if (width < mk) return dn::fail(DN_E_INVALID, "dn_bam_rows_keys: width below the longest key (" + std::to_string(mk) + ")");
        DN_TRY(alloc_padded(d_keys, (size_t) (h->n_rows * width)));
        hipLaunchKernelGGL(k_bam_keys, dim3(dn::grid_for(h->n_rows, kNT, kGridCap)), dim3(kNT), 0, h->st, h->n_rows, h->name_beg.get(), h->key_len.get(),
                           h->names.get(), width, d_keys.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(keys, d_keys, (size_t) (h->n_rows * width), hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    });
}

extern "C" int dn_bam_rows_fetch(dn_bam_rows h, int64_t *pos, int64_t *op_beg, int32_t *n_op, uint32_t *ops, int64_t *name_beg,
                                 int32_t *name_len, uint8_t *names)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_rows_fetch: bad argument");
    hipStream_t st = h->st;
    const size_t n = (size_t) h->n_rows;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(st, [&]() -> int {
        if (n > 0) {
            if (pos) DN_TRY(hipMemcpyAsync(pos, h->pos, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
            if (op_beg) DN_TRY(hipMemcpyAsync(op_beg, h->op_beg, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
            if (n_op) DN_TRY(hipMemcpyAsync(n_op, h->n_op, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
            if (name_beg) DN_TRY(hipMemcpyAsync(name_beg, h->name_beg, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
            if (name_len) DN_TRY(hipMemcpyAsync(name_len, h->name_len, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        }
        if (ops && h->n_ops > 0) DN_TRY(hipMemcpyAsync(ops, h->ops, sizeof(uint32_t) * (size_t) h->n_ops, hipMemcpyDeviceToHost, st));
        if (names && h->n_names > 0) DN_TRY(hipMemcpyAsync(names, h->names, (size_t) h->n_names, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        return DN_OK;
    });
}

extern "C" int dn_bam_rows_pair(dn_bam_rows h, int32_t *order_out, int32_t *pair_id_out, int64_t *n_pair_ids, double *device_ms)
{
    dn::clear_error();
    if (!h || !h->F.paired || h->n_rows > INT32_MAX) return dn::fail(DN_E_INVALID, "dn_bam_rows_pair: bad argument (a paired store of fewer than 2^31 rows)");
    const int64_t n = h->n_rows;
    hipStream_t st = h->st;
    int32_t mk = 0, last_id = -1;                    // what the stream copies to the host
    dn::PairWork work;
    dn::Event e0, e1;
    h->has_pairing = false;
    h->n_pair_ids = 0;
    if (n_pair_ids) *n_pair_ids = 0;
    if (device_ms) *device_ms = 0.0;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(st, [&]() -> int {
        if (n > 0) {
            DN_TRY(e0.create(hipEventCreate));
            DN_TRY(e1.create(hipEventCreate));
            DN_TRY(hipMemcpyAsync(&mk, h->max_key, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            DN_TRY(hipStreamSynchronize(st));
            DN_TRY(alloc_padded(h->pair_order, (size_t) n)); DN_TRY(alloc_padded(h->pair_id, (size_t) n));
            DN_TRY(hipEventRecord(e0, st));
            dn::MateCoords mates;
            if (h->F.by_flag) { mates.pos = h->pos; mates.next_pos = h->next_pos; mates.flag = h->flag; }
            const int rc = dn::pair_device(st, n, mk, h->name_beg, h->key_len, h->names, mates, work, h->pair_order, h->pair_id);
            if (rc != DN_OK) return rc;
            DN_TRY(hipEventRecord(e1, st));
            DN_TRY(hipMemcpyAsync(&last_id, h->pair_id + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
            if (order_out) DN_TRY(hipMemcpyAsync(order_out, h->pair_order, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
            if (pair_id_out) DN_TRY(hipMemcpyAsync(pair_id_out, h->pair_id, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
            DN_TRY(hipStreamSynchronize(st));
            if (device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *device_ms = ms; }
            h->n_pair_ids = (int64_t) last_id + 1;
        }
        h->has_pairing = true;
        if (n_pair_ids) *n_pair_ids = h->n_pair_ids;
        return DN_OK;
    });
}

extern "C" int dn_bam_rows_set_stranded(dn_bam_rows h, int32_t stranded)
{
    dn::clear_error();
    if (!h || (stranded != dn::kStrandNo && stranded != dn::kStrandForward && stranded != dn::kStrandReverse))
        return dn::fail(DN_E_INVALID, "dn_bam_rows_set_stranded: bad argument (stranded 0, no, 1, forward, or 2, reverse)");
    if (h->n_rows > 0 && stranded != h->stranded)
        return dn::fail(DN_E_STATE, "dn_bam_rows_set_stranded: the store already has rows");
    h->stranded = stranded;
    return DN_OK;
}

extern "C" int dn_bam_rows_fetch_sense(dn_bam_rows h, uint8_t *sense)
{
    dn::clear_error();
    if (!h || h->stranded == dn::kStrandNo || (h->n_rows > 0 && !sense))
        return dn::fail(DN_E_INVALID, "dn_bam_rows_fetch_sense: bad argument (a stranded store)");
    if (h->n_rows == 0) return DN_OK;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(hipMemcpyAsync(sense, h->sense, (size_t) h->n_rows, hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    });
}

// dn_bam_rows_coverage, and with strand != 0 dn_bam_rows_coverage_strand on the rows of that sense
static int rows_coverage(dn_bam_rows h, uint8_t strand, const int32_t *order, const int32_t *pair_id, int64_t n_pair_ids, const CoverageIO &io)
{
    const bool resident = h->F.paired && h->n_rows > 0 && !order && !pair_id && h->has_pairing;     // the pairing of dn_bam_rows_pair
    if (h->F.paired && h->n_rows > 0 && !order && !resident) return dn::fail(DN_E_INVALID, "dn_bam_rows_coverage: bad argument");
    if (h->F.by_flag && h->n_rows > 0 && !resident)
        return dn::fail(DN_E_INVALID, "dn_bam_rows_coverage: a store that pairs by FLAG takes the pairing of dn_bam_rows_pair (order and pair_id NULL)");
    MateBits mate_bits;
    if (h->F.by_flag && resident) { mate_bits.flag = h->flag; mate_bits.order = h->pair_order; }
    if (h->has_no_cigar) return dn::fail(DN_E_INVALID, "read " + h->no_cigar + " has no CIGAR string");     // the reference's CIGAR regex on cigarstring None
    StrandSel sel;
    if (strand) { sel.sense = h->sense; sel.want = strand; }
    const int64_t n = h->n_rows;
    hipStream_t st = h->st;
    std::vector<int32_t> h_order;
    dn::DeviceBuffer<int64_t> g_pos, g_beg;
    dn::DeviceBuffer<int32_t> g_cnt, d_order;
    const int64_t *p_pos = h->pos, *p_beg = h->op_beg;
    const int32_t *p_cnt = h->n_op;
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(st, [&]() -> int {
        if (order && n > 0) {                                   // rows in the caller's order (paired: the sort by qname_unpaired)
            h_order.assign(order, order + n);
            for (int64_t r = 0; r < n; r++)
                if (order[r] < 0 || order[r] >= n) return dn::fail(DN_E_INVALID, "dn_bam_rows_coverage: order out of range");
            DN_TRY(alloc_padded(d_order, n)); DN_TRY(alloc_padded(g_pos, n)); DN_TRY(alloc_padded(g_beg, n)); DN_TRY(alloc_padded(g_cnt, n));
            DN_TRY(hipMemcpyAsync(d_order, order, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_bam_gather, dim3(dn::grid_for(n, kNT, kGridCap)), dim3(kNT), 0, st, n, d_order.get(), h->pos.get(), h->op_beg.get(),
                               h->n_op.get(), g_pos.get(), g_beg.get(), g_cnt.get());
            DN_TRY(hipGetLastError());
            p_pos = g_pos; p_beg = g_beg; p_cnt = g_cnt;
            sel.order = d_order;
        } else if (resident) {                                // the same rows in the store's own order: nothing to check or upload
            DN_TRY(alloc_padded(g_pos, n)); DN_TRY(alloc_padded(g_beg, n)); DN_TRY(alloc_padded(g_cnt, n));
            hipLaunchKernelGGL(k_bam_gather, dim3(dn::grid_for(n, kNT, kGridCap)), dim3(kNT), 0, st, n, (const int32_t *) h->pair_order.get(), h->pos.get(),
                               h->op_beg.get(), h->n_op.get(), g_pos.get(), g_beg.get(), g_cnt.get());
            DN_TRY(hipGetLastError());
            p_pos = g_pos; p_beg = g_beg; p_cnt = g_cnt;
            sel.order = h->pair_order;
        }
        return coverage_stages(st, h->F.paired, n, p_pos, BamCigars{p_beg, p_cnt, h->ops}, pair_id, resident ? h->pair_id.get() : nullptr,
                               resident ? h->n_pair_ids : n_pair_ids, io, [&](int64_t r) {
            int64_t s = h_order.empty() ? r : h_order[r];
            if (resident) {
                int32_t o = -1;
                if (hipMemcpy(&o, h->pair_order + r, sizeof(o), hipMemcpyDeviceToHost) != hipSuccess || o < 0 || o >= n) return std::string("?");
                s = o;
            }
            int64_t beg = 0;
            int32_t cnt = 0;
            std::vector<uint32_t> ops;
            std::string name;
            if (hipMemcpy(&beg, h->op_beg + s, sizeof(beg), hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(&cnt, h->n_op + s, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess && cnt >= 0) {
                ops.resize((size_t) cnt);
                if (cnt > 0 && hipMemcpy(ops.data(), h->ops + beg, sizeof(uint32_t) * (size_t) cnt, hipMemcpyDeviceToHost) != hipSuccess) ops.clear();
            }
            int64_t nb = 0;
            int32_t nl = 0;
            if (hipMemcpy(&nb, h->name_beg + s, sizeof(nb), hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(&nl, h->name_len + s, sizeof(nl), hipMemcpyDeviceToHost) == hipSuccess && nl > 0) {
                name.resize((size_t) nl);
                if (hipMemcpy(&name[0], h->names + nb, (size_t) nl, hipMemcpyDeviceToHost) != hipSuccess) name = "?";
            }
            return cigar_string(ops.data(), (int64_t) ops.size()) + " (read " + name + ")";
        }, mate_bits, sel);
    });
}

extern "C" int dn_bam_rows_coverage(dn_bam_rows h, const int32_t *order, const int32_t *pair_id, int64_t n_pair_ids,
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
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_rows_coverage: bad argument");
    COVERAGE_IO;
    return rows_coverage(h, 0, order, pair_id, n_pair_ids, io);
}

extern "C" int dn_bam_rows_coverage_strand(dn_bam_rows h, int32_t strand, const int32_t *order, const int32_t *pair_id, int64_t n_pair_ids,
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
    dn::clear_error();
    if (!h || h->stranded == dn::kStrandNo || !strand_selector(strand))
        return dn::fail(DN_E_INVALID, "dn_bam_rows_coverage_strand: bad argument (a stranded store, and the strand '+' or '-')");
    COVERAGE_IO;
    return rows_coverage(h, strand_selector(strand), order, pair_id, n_pair_ids, io);
}

extern "C" int dn_bam_cigar_bounds(int device, int64_t n, const int64_t *pos, const int64_t *op_off, const uint32_t *ops,
                                   int32_t max_seg, int32_t *nseg, int64_t *bounds, int64_t *end_pos)
{
    dn::clear_error();
    if (n < 0 || max_seg < 1 || max_seg > kMaxSeg || (n > 0 && (!pos || !op_off || !nseg || !bounds || !end_pos)))
        return dn::fail(DN_E_INVALID, "dn_bam_cigar_bounds: bad argument");
    if (n == 0) return DN_OK;
    const int64_t n_ops = op_off[n];
    std::vector<int32_t> cnt((size_t) n);
    for (int64_t r = 0; r < n; r++) {
        if (op_off[r + 1] < op_off[r] || op_off[r] < 0 || op_off[r + 1] - op_off[r] > INT32_MAX)
            return dn::fail(DN_E_INVALID, "dn_bam_cigar_bounds: bad op_off");
        cnt[(size_t) r] = (int32_t) (op_off[r + 1] - op_off[r]);
    }
    if (n_ops > 0 && !ops) return dn::fail(DN_E_INVALID, "dn_bam_cigar_bounds: bad argument");
    dn::DeviceBuffer<int64_t> d_beg;
    dn::DeviceBuffer<int32_t> d_cnt;
    dn::DeviceBuffer<uint32_t> d_ops;
    dn::Stream st;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(alloc_padded(d_beg, n)); DN_TRY(alloc_padded(d_cnt, n)); DN_TRY(alloc_padded(d_ops, n_ops));
        DN_TRY(hipMemcpyAsync(d_beg, op_off, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_cnt, cnt.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, st));
        if (n_ops > 0) DN_TRY(hipMemcpyAsync(d_ops, ops, sizeof(uint32_t) * (size_t) n_ops, hipMemcpyHostToDevice, st));
        return cigar_debug(st, n, pos, BamCigars{d_beg, d_cnt, d_ops}, max_seg, nseg, bounds, end_pos);
    });
}

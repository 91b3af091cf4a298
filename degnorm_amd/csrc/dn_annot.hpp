// dn_annot.hpp -- the exon table of the two annotation scans (dn_gtf.hip, dn_gff3.hip): the columns of the lines of a window
// (one entry per line, written by the unit's parse kernel next to a kind byte per line), of the exon rows that go to the host
// and of the GFF3 node store; their owner, the compaction of the lines of one kind to rows in file order, and the copies of
// the rows to the caller.  c is the chromosome name (a node's ID), a the gene name (or the Parent still to resolve).
#pragma once
#include "dn_lines.hpp"
#include "dn_fields.hpp"

namespace {

struct ExonCols {
    int64_t *line, *c_beg, *start, *end, *a_beg;
    int32_t *c_len, *a_len;
    uint64_t *c_hash, *a_hash;
    uint8_t *open;                      // 1: a is a Parent.  Null where no row is open (GTF)
};

constexpr unsigned long long kNoFasta = ~0ull;         // the line of ##FASTA in a text that has none

// is line j of the window (line_base + j + 1 of the file) of kind `which` and above the ##FASTA line?
__device__ inline bool kept_as(int which, const uint8_t *__restrict__ kind, int64_t j, int64_t n_lanes, int64_t line_base, unsigned long long fasta)
{
    return j < n_lanes && kind[j] == (uint8_t) which && (unsigned long long) (line_base + j + 1) < fasta;
}

template <class T> __device__ inline void put(T *dst, int64_t r, const T *src, int64_t j)
{
    if (dst) dst[r] = src[j];
}

// The lines that are kept_as `which` (first_fasta null: the text has no ##FASTA rule) to rows [0, n_rows) of `row`, in file
// order: block offset + rank inside the block.  A column is copied when `row` has it: a node row has no line, start and end.
__global__ __launch_bounds__(kNT) void k_compact(int which, const uint8_t *__restrict__ kind, int64_t n_lanes, int64_t line_base,
                                                  const unsigned long long *__restrict__ first_fasta, const int64_t *__restrict__ block_off,
                                                  ExonCols rec, ExonCols row, int64_t n_rows)
{
    const int64_t j = (int64_t) blockIdx.x * kNT + threadIdx.x;
    const int kept = kept_as(which, kind, j, n_lanes, line_base, first_fasta ? *first_fasta : kNoFasta) ? 1 : 0;
    int total;
    const int64_t r = block_off[blockIdx.x] + block_exclusive(kept, &total);
    if (!kept || r < 0 || r >= n_rows) return;
    put(row.line, r, rec.line, j);
    put(row.c_beg, r, rec.c_beg, j);
    put(row.c_len, r, rec.c_len, j);
    put(row.c_hash, r, rec.c_hash, j);
    put(row.start, r, rec.start, j);
    put(row.end, r, rec.end, j);
    put(row.a_beg, r, rec.a_beg, j);
    put(row.a_len, r, rec.a_len, j);
    put(row.a_hash, r, rec.a_hash, j);
    put(row.open, r, rec.open, j);
}

// The optional strand column of both scans (dn::strand_field, dn_fields.hpp), two small kernels that run only when the caller
// asks for it, while the window's text is resident; the parse kernels and k_compact know nothing of it.
// k_strand_check: one lane per line, as the parse kernel (lane j takes line n_head + j of the table): an exon line whose field
// seven is not one of + - . ? is reported as `err_kind` to the word the parse kernel reports to, so the first faulty line wins
// whatever its fault.
__global__ __launch_bounds__(kNT) void k_strand_check(const uint8_t *__restrict__ buf, int64_t limit, const int64_t *__restrict__ line_start,
                                                       int64_t n_starts, int64_t n_head, int64_t line_base, const uint8_t *__restrict__ kind,
                                                       int err_kind, unsigned long long *__restrict__ first_error)
{
    const int64_t j = (int64_t) blockIdx.x * kNT + threadIdx.x, i = n_head + j;
    if (i >= n_starts || kind[j] != (uint8_t) dn::kExon) return;
    int64_t beg, end;
    line_span(line_start, n_starts, limit, i, &beg, &end);
    Bytes b(buf);
    if (beg < 0 || end > limit || !dn::strand_field(b, beg, end)) report_error(first_error, line_base + j + 1, err_kind);
}

// k_row_strand: one lane per exon row, after compaction: from the row's line start (c_beg, an offset into buf) to field seven.
__global__ __launch_bounds__(kNT) void k_row_strand(const uint8_t *__restrict__ buf, int64_t limit, const int64_t *__restrict__ c_beg,
                                                     int64_t n_rows, uint8_t *__restrict__ strand)
{
    const int64_t r = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (r >= n_rows) return;
    Bytes b(buf);
    const int64_t beg = c_beg[r];
    strand[r] = beg >= 0 && beg < limit ? dn::strand_field(b, beg, limit) : 0;
}

struct ExonBuffers {
    dn::DeviceBuffer<int64_t> line, c_beg, start, end, a_beg;
    dn::DeviceBuffer<int32_t> c_len, a_len;
    dn::DeviceBuffer<uint64_t> c_hash, a_hash;
    dn::DeviceBuffer<uint8_t> open;
    hipError_t alloc(int64_t n, bool with_open)
    {
        const size_t m = (size_t) (n > 0 ? n : 1);
        hipError_t e = hipSuccess;
        for (dn::DeviceBuffer<int64_t> *b : {&line, &c_beg, &start, &end, &a_beg})
            if (e == hipSuccess) e = b->alloc(m * sizeof(int64_t));
        for (dn::DeviceBuffer<int32_t> *b : {&c_len, &a_len})
            if (e == hipSuccess) e = b->alloc(m * sizeof(int32_t));
        for (dn::DeviceBuffer<uint64_t> *b : {&c_hash, &a_hash})
            if (e == hipSuccess) e = b->alloc(m * sizeof(uint64_t));
        if (e == hipSuccess && with_open) e = open.alloc(m);
        return e;
    }
    ExonCols view() const { return ExonCols{line, c_beg, start, end, a_beg, c_len, a_len, c_hash, a_hash, open}; }
};

template <class T> hipError_t rows_out(hipStream_t st, T *dst, const T *src, int64_t n, hipError_t e)
{
    return e == hipSuccess && dst && n > 0 ? hipMemcpyAsync(dst, src, sizeof(T) * (size_t) n, hipMemcpyDeviceToHost, st) : e;
}

// queues the copies of rows [0, n) of the device columns `row` to the caller's columns `out`; a null column of `out` is left out
inline hipError_t copy_rows(hipStream_t st, const ExonCols &out, const ExonCols &row, int64_t n)
{
    hipError_t e = rows_out(st, out.line, row.line, n, hipSuccess);
    e = rows_out(st, out.c_beg, row.c_beg, n, e);
    e = rows_out(st, out.c_len, row.c_len, n, e);
    e = rows_out(st, out.c_hash, row.c_hash, n, e);
    e = rows_out(st, out.start, row.start, n, e);
    e = rows_out(st, out.end, row.end, n, e);
    e = rows_out(st, out.a_beg, row.a_beg, n, e);
    e = rows_out(st, out.a_len, row.a_len, n, e);
    e = rows_out(st, out.a_hash, row.a_hash, n, e);
    return rows_out(st, out.open, row.open, n, e);
}

}  // namespace

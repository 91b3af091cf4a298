// dn_gtf.hip -- GTF annotation scan on the device (GeneAnnotationLoader, degnorm_amd/loaders.py; dn_gtf.hpp holds the rule of a
// line).
//
// Replaces the reference's read_csv + two `apply` passes per row (loaders.py:128-152): the raw bytes of a GTF file, or of a
// window of it that ends at a line end, go to the GPU and come back as the table of its exon lines in file order.
//   1  k_count_newlines, k_scan, k_line_starts   where every line starts (LineTable, dn_lines.hpp, shared with dn_gff3.hip
//                         and dn_sam.hip)
//   2  k_parse_lines      one lane per line (gtf::parse_line): skip rule, the first eight tabs, `exon`, start / end, the gene
//                         name; a record and a kind byte per line, kept lines per 256-line block, the first malformed line
//                         by atomicMin
//   3  k_scan             prefix sum of the per-block kept counts
//   4  k_compact          kept records to their rows: block offset + rank inside the block, so rows are in file order
//                         (dn_annot.hpp, shared with dn_gff3.hip)
// Every byte is read through Bytes: aligned 8-byte words of a buffer that is zero-padded to whole tiles, and only at
// positions below the line's end, which is at most n_bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_annot.hpp"
#include "dn_gtf.hpp"

namespace {

__global__ __launch_bounds__(kNT) void k_parse_lines(const uint8_t *__restrict__ buf, int64_t n_bytes, const int64_t *__restrict__ line_start,
                                                      int64_t n_starts, ExonCols rec, uint8_t *__restrict__ kind, int32_t *__restrict__ block_kept,
                                                      unsigned long long *__restrict__ first_error)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    int kept = 0;
    if (i < n_starts) {
        int64_t beg, end;
        line_span(line_start, n_starts, n_bytes, i, &beg, &end);
        Bytes b(buf);
        int64_t chr_end = 0, start = 0, stop = 0, g_lo = 0, g_hi = 0;
        const int r = beg <= end && end <= n_bytes ? dn::gtf::parse_line(b, beg, end, &chr_end, &start, &stop, &g_lo, &g_hi) : dn::kSkip;
        if (r < 0) report_error(first_error, i + 1, -r);
        kept = r == dn::kExon;
        if (kept) {
            rec.line[i] = i + 1;
            rec.c_beg[i] = beg;
            rec.c_len[i] = (int32_t) (chr_end - beg);
            rec.c_hash[i] = dn::fnv1a(b, beg, chr_end);
            rec.start[i] = start;
            rec.end[i] = stop;
            rec.a_beg[i] = g_lo;
            rec.a_len[i] = (int32_t) (g_hi - g_lo);
            rec.a_hash[i] = dn::fnv1a(b, g_lo, g_hi);
        }
        kind[i] = (uint8_t) (kept ? dn::kExon : dn::kSkip);
    }
    int total;
    (void) block_exclusive(kept, &total);
    if (threadIdx.x == 0) block_kept[blockIdx.x] = total;
}

}  // namespace

// dn_gtf_scan, and with `strand` not null dn_gtf_scan_strand: field seven of every exon row, checked before the rows are the caller's
static int gtf_scan(int device, const uint8_t *buf, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                    int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                    int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *strand, int64_t *err_line, int32_t *err_kind,
                    double *copy_ms, double *device_ms)
{
    if (!buf || n_bytes < 1 || row_cap < 0 || !n_lines || !n_rows || !line || !chr_beg || !chr_len || !chr_hash || !start || !end
        || !gene_beg || !gene_len || !gene_hash || !err_line || !err_kind)
        return dn::fail(DN_E_INVALID, "dn_gtf_scan: bad argument");
    const int64_t n_tiles = (n_bytes + kTile - 1) / kTile, padded = n_tiles * kTile;
    *n_lines = 0; *n_rows = 0; *err_line = 0; *err_kind = 0;
    // what the stream reads or writes: owned here, so that it outlives the wait of dn::synced
    dn::Stream st;
    dn::Event e0, e1, e2;
    dn::DeviceBuffer<uint8_t> d_buf, d_kind, d_strand;
    dn::DeviceBuffer<int32_t> d_block_kept;
    dn::DeviceBuffer<int64_t> d_block_off;
    dn::DeviceBuffer<unsigned long long> d_err;
    LineTable lines;
    ExonBuffers rec, row;
    unsigned long long first_error = kNoError;
    int64_t kept = 0;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(e2.create(hipEventCreate));
        DN_TRY(d_buf.alloc((size_t) padded));
        DN_TRY(lines.alloc(n_tiles));
        DN_TRY(d_err.alloc(sizeof(unsigned long long)));
        DN_TRY(hipEventRecord(e0, st));
        DN_TRY(upload_padded(st, d_buf, buf, n_bytes, padded));
        DN_TRY(hipMemcpyAsync(d_err, &kNoError, sizeof(kNoError), hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));

        const int rc = lines.find(st, d_buf, n_tiles, 0, n_bytes, "dn_gtf_scan");
        if (rc != DN_OK) return rc;
        const int64_t n_starts = lines.n_starts;
        const int64_t n_blocks = (n_starts + kNT - 1) / kNT;
        DN_TRY(d_kind.alloc((size_t) n_starts));
        DN_TRY(d_block_kept.alloc(sizeof(int32_t) * (size_t) n_blocks));
        DN_TRY(d_block_off.alloc(sizeof(int64_t) * (size_t) n_blocks));
        DN_TRY(rec.alloc(n_starts, false));
        hipLaunchKernelGGL(k_parse_lines, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_bytes,
                           (const int64_t *) lines.line_start.get(), n_starts, rec.view(), d_kind.get(), d_block_kept.get(), d_err.get());
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanNT), 0, st, d_block_kept.get(), n_blocks, d_block_off.get(), lines.total.get());
        if (strand)
            hipLaunchKernelGGL(k_strand_check, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_bytes,
                               (const int64_t *) lines.line_start.get(), n_starts, (int64_t) 0, (int64_t) 0, (const uint8_t *) d_kind.get(),
                               (int) DN_GTF_E_STRAND, d_err.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&kept, lines.total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(&first_error, d_err, sizeof(first_error), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));

        *n_lines = lines.n_newlines + (buf[n_bytes - 1] != '\n' ? 1 : 0);
        if (unpack_error(first_error, err_line, err_kind)) {
            DN_TRY(hipEventRecord(e2, st));
        } else {
            if (kept < 0 || kept > row_cap) return dn::fail(DN_E_INVALID, "dn_gtf_scan: more exon lines than the caller's tables hold");
            DN_TRY(row.alloc(kept, false));
            if (kept > 0) {
                hipLaunchKernelGGL(k_compact, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (int) dn::kExon, (const uint8_t *) d_kind.get(), n_starts,
                                   (int64_t) 0, (const unsigned long long *) nullptr, (const int64_t *) d_block_off.get(), rec.view(), row.view(), kept);
                DN_TRY(hipGetLastError());
            }
            if (strand && kept > 0) {                               // while the window is resident
                DN_TRY(d_strand.alloc((size_t) kept));
                hipLaunchKernelGGL(k_row_strand, dim3((unsigned) ((kept + kNT - 1) / kNT)), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_bytes,
                                   (const int64_t *) row.c_beg.get(), kept, d_strand.get());
                DN_TRY(hipGetLastError());
            }
            DN_TRY(hipEventRecord(e2, st));
            if (strand && kept > 0) DN_TRY(hipMemcpyAsync(strand, d_strand, (size_t) kept, hipMemcpyDeviceToHost, st));
            DN_TRY(copy_rows(st, ExonCols{line, chr_beg, start, end, gene_beg, chr_len, gene_len, chr_hash, gene_hash, nullptr}, row.view(), kept));
            *n_rows = kept;
        }
        DN_TRY(hipStreamSynchronize(st));
        if (copy_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *copy_ms = ms; }
        if (device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *device_ms = ms; }
        return DN_OK;
    });
}

extern "C" int dn_gtf_scan(int device, const uint8_t *buf, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                           int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                           int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, int64_t *err_line, int32_t *err_kind,
                           double *copy_ms, double *device_ms)
{
    return gtf_scan(device, buf, n_bytes, row_cap, n_lines, n_rows, line, chr_beg, chr_len, chr_hash, start, end, gene_beg, gene_len, gene_hash,
                    nullptr, err_line, err_kind, copy_ms, device_ms);
}

extern "C" int dn_gtf_scan_strand(int device, const uint8_t *buf, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                                  int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                                  int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *strand, int64_t *err_line,
                                  int32_t *err_kind, double *copy_ms, double *device_ms)
{
    return gtf_scan(device, buf, n_bytes, row_cap, n_lines, n_rows, line, chr_beg, chr_len, chr_hash, start, end, gene_beg, gene_len, gene_hash,
                    strand, err_line, err_kind, copy_ms, device_ms);
}

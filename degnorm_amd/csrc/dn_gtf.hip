// dn_gtf.hip -- GTF annotation scan on the device (GeneAnnotationLoader, degnorm_amd/loaders.py).
//
// Replaces the reference's read_csv + two `apply` passes per row (loaders.py:128-152): the raw bytes of a GTF file, or of a
// window of it that ends at a line end, go to the GPU and come back as the table of its exon lines in file order.
//   1  k_count_newlines   '\n' per 16 KiB tile (four 16-byte loads per lane)
//   2  k_scan             exclusive prefix sum of the tile counts (one workgroup)
//   3  k_line_starts      the byte offset every line starts at
//   4  k_parse_lines      one lane per line: skip rule, the first eight tabs, `exon`, start / end, the gene name; a record
//                         and a keep flag per line, kept lines per 256-line block, the first malformed line by atomicMin
//   5  k_scan             prefix sum of the per-block kept counts
//   6  k_compact          kept records to their rows: block offset + rank inside the block, so rows are in file order
// Passes 1 to 3 and Bytes are those of dn_lines.hpp, which the SAM encoder (dn_sam.hip) shares.
// Every byte is read through Bytes: aligned 8-byte words of a buffer that is zero-padded to whole tiles, and only at
// positions below the line's end, which is at most n_bytes.  Every loop ends at the line's end or before.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_lines.hpp"

namespace {

// the records of the lines (one per line) and of the rows (one per kept line)
struct Table {
    int64_t *line, *chr_beg, *start, *end, *gene_beg;
    int32_t *chr_len, *gene_len;
    uint64_t *chr_hash, *gene_hash;
};

__device__ inline uint64_t fnv1a(Bytes &b, int64_t lo, int64_t hi)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t p = lo; p < hi; p++) h = (h ^ b.at(p)) * 0x100000001b3ull;
    return h;
}

// [lo, hi) as a decimal integer of 1 .. 18 digits and nothing else
__device__ inline bool parse_int(Bytes &b, int64_t lo, int64_t hi, int64_t *out)
{
    if (hi <= lo || hi - lo > 18) return false;
    int64_t v = 0;
    for (int64_t p = lo; p < hi; p++) {
        const uint32_t c = b.at(p);
        if (c < '0' || c > '9') return false;
        v = v * 10 + (int64_t) (c - '0');
    }
    *out = v;
    return true;
}

// does [p, end) begin with tag (n bytes)?
__device__ inline bool begins_with(Bytes &b, int64_t p, int64_t end, const char *tag, int n)
{
    if (end - p < n) return false;
    for (int k = 0; k < n; k++)
        if (b.at(p + k) != (uint32_t) tag[k]) return false;
    return true;
}

// [*lo, *hi) without blanks and double quotes at either end
__device__ inline void strip_value(Bytes &b, int64_t *lo, int64_t *hi)
{
    int64_t a = *lo, z = *hi;
    while (a < z) { const uint32_t c = b.at(a); if (c != ' ' && c != '"') break; a++; }
    while (z > a) { const uint32_t c = b.at(z - 1); if (c != ' ' && c != '"') break; z--; }
    *lo = a; *hi = z;
}

// The gene name of attribute field [a, end): pieces between ';', blanks stripped; the first piece that begins with gene_name
// gives it, and when there is none or its value is empty the first piece that begins with gene_id (loaders.py:102-112).
// The field ends at a tab as well.  False: neither gives a value.
__device__ inline bool gene_of(Bytes &b, int64_t a, int64_t end, int64_t *g_lo, int64_t *g_hi)
{
    bool seen_name = false, seen_id = false;
    int64_t id_lo = 0, id_hi = 0;
    int64_t p = a;
    while (p < end) {
        while (p < end && b.at(p) == ' ') p++;
        const bool is_name = !seen_name && begins_with(b, p, end, "gene_name", 9);
        const bool is_id = !seen_id && !is_name && begins_with(b, p, end, "gene_id", 7);
        int64_t q = p;
        uint32_t c = 0;
        while (q < end) { c = b.at(q); if (c == ';' || c == '\t') break; q++; }
        if (is_name) {
            int64_t lo = p + 9, hi = q;
            strip_value(b, &lo, &hi);
            if (hi > lo) { *g_lo = lo; *g_hi = hi; return true; }
            seen_name = true;
        } else if (is_id) {
            id_lo = p + 7; id_hi = q;
            strip_value(b, &id_lo, &id_hi);
            seen_id = true;
        }
        if (q >= end || c == '\t' || (seen_name && seen_id)) break;
        p = q + 1;
    }
    if (seen_id && id_hi > id_lo) { *g_lo = id_lo; *g_hi = id_hi; return true; }
    return false;
}

// 0: the line is skipped, 1: kept (rec filled), < 0: -(DN_GTF_E_*)
__device__ inline int parse_line(Bytes &b, int64_t beg, int64_t end, int64_t *chr_end, int64_t *start, int64_t *stop, int64_t *g_lo, int64_t *g_hi)
{
    if (end > beg && b.at(end - 1) == '\r') end--;
    if (end <= beg || b.at(beg) == '#') return 0;
    int64_t t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t8 = 0;
    int nt = 0;
    for (int64_t p = beg; p < end; p++) {
        if (b.at(p) != '\t') continue;
        nt++;
        if (nt == 1) t1 = p;
        else if (nt == 2) t2 = p;
        else if (nt == 3) t3 = p;
        else if (nt == 4) t4 = p;
        else if (nt == 5) t5 = p;
        else if (nt == 8) { t8 = p; break; }
    }
    if (nt < 8) return -DN_GTF_E_FIELDS;
    if (t3 - t2 - 1 != 4) return 0;
    const char exon[4] = {'e', 'x', 'o', 'n'};
    for (int k = 0; k < 4; k++)
        if ((b.at(t2 + 1 + k) | 0x20u) != (uint32_t) exon[k]) return 0;
    if (!parse_int(b, t3 + 1, t4, start) || !parse_int(b, t4 + 1, t5, stop)) return -DN_GTF_E_INTEGER;
    if (!gene_of(b, t8 + 1, end, g_lo, g_hi)) return -DN_GTF_E_GENE;
    *chr_end = t1;
    return 1;
}

__global__ __launch_bounds__(kNT) void k_parse_lines(const uint8_t *__restrict__ buf, int64_t n_bytes, const int64_t *__restrict__ line_start,
                                                      int64_t n_starts, Table rec, uint8_t *__restrict__ keep, int32_t *__restrict__ block_kept,
                                                      unsigned long long *__restrict__ first_error)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    int kept = 0;
    if (i < n_starts) {
        const int64_t beg = line_start[i];
        const int64_t end = i + 1 < n_starts ? line_start[i + 1] - 1 : n_bytes;
        Bytes b(buf);
        int64_t chr_end = 0, start = 0, stop = 0, g_lo = 0, g_hi = 0;
        const int r = beg <= end && end <= n_bytes ? parse_line(b, beg, end, &chr_end, &start, &stop, &g_lo, &g_hi) : 0;
        if (r < 0) atomicMin(first_error, ((unsigned long long) (i + 1) << 8) | (unsigned long long) (-r));
        kept = r == 1;
        if (kept) {
            rec.line[i] = i + 1;
            rec.chr_beg[i] = beg;
            rec.chr_len[i] = (int32_t) (chr_end - beg);
            rec.chr_hash[i] = fnv1a(b, beg, chr_end);
            rec.start[i] = start;
            rec.end[i] = stop;
            rec.gene_beg[i] = g_lo;
            rec.gene_len[i] = (int32_t) (g_hi - g_lo);
            rec.gene_hash[i] = fnv1a(b, g_lo, g_hi);
        }
        keep[i] = (uint8_t) kept;
    }
    int total;
    (void) block_exclusive(kept, &total);
    if (threadIdx.x == 0) block_kept[blockIdx.x] = total;
}

__global__ __launch_bounds__(kNT) void k_compact(int64_t n_starts, const uint8_t *__restrict__ keep, const int64_t *__restrict__ block_off,
                                                  Table rec, Table row, int64_t n_rows)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    const int kept = i < n_starts ? keep[i] : 0;
    int total;
    const int64_t r = block_off[blockIdx.x] + block_exclusive(kept, &total);
    if (!kept || r >= n_rows) return;
    row.line[r] = rec.line[i];
    row.chr_beg[r] = rec.chr_beg[i];
    row.chr_len[r] = rec.chr_len[i];
    row.chr_hash[r] = rec.chr_hash[i];
    row.start[r] = rec.start[i];
    row.end[r] = rec.end[i];
    row.gene_beg[r] = rec.gene_beg[i];
    row.gene_len[r] = rec.gene_len[i];
    row.gene_hash[r] = rec.gene_hash[i];
}

struct TableBuffers {
    dn::DeviceBuffer<int64_t> line, chr_beg, start, end, gene_beg;
    dn::DeviceBuffer<int32_t> chr_len, gene_len;
    dn::DeviceBuffer<uint64_t> chr_hash, gene_hash;
    hipError_t alloc(int64_t n)
    {
        const size_t m = (size_t) (n > 0 ? n : 1);
        hipError_t e = hipSuccess;
        for (dn::DeviceBuffer<int64_t> *b : {&line, &chr_beg, &start, &end, &gene_beg})
            if (e == hipSuccess) e = b->alloc(m * sizeof(int64_t));
        for (dn::DeviceBuffer<int32_t> *b : {&chr_len, &gene_len})
            if (e == hipSuccess) e = b->alloc(m * sizeof(int32_t));
        for (dn::DeviceBuffer<uint64_t> *b : {&chr_hash, &gene_hash})
            if (e == hipSuccess) e = b->alloc(m * sizeof(uint64_t));
        return e;
    }
    Table view() const { return Table{line, chr_beg, start, end, gene_beg, chr_len, gene_len, chr_hash, gene_hash}; }
};

}  // namespace

extern "C" int dn_gtf_scan(int device, const uint8_t *buf, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                           int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                           int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, int64_t *err_line, int32_t *err_kind,
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
    dn::DeviceBuffer<uint8_t> d_buf, d_keep;
    dn::DeviceBuffer<int32_t> d_tile_count, d_block_kept;
    dn::DeviceBuffer<int64_t> d_tile_off, d_block_off, d_line_start, d_total;
    dn::DeviceBuffer<unsigned long long> d_err;
    TableBuffers rec, row;
    const unsigned long long no_error = ~0ull;
    unsigned long long first_error = no_error;
    int64_t n_newlines = 0, kept = 0;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(e2.create(hipEventCreate));
        DN_TRY(d_buf.alloc((size_t) padded));
        DN_TRY(d_tile_count.alloc(sizeof(int32_t) * (size_t) n_tiles));
        DN_TRY(d_tile_off.alloc(sizeof(int64_t) * (size_t) n_tiles));
        DN_TRY(d_total.alloc(sizeof(int64_t)));
        DN_TRY(d_err.alloc(sizeof(unsigned long long)));
        DN_TRY(hipEventRecord(e0, st));
        DN_TRY(hipMemcpyAsync(d_buf, buf, (size_t) n_bytes, hipMemcpyHostToDevice, st));
        if (padded > n_bytes) DN_TRY(hipMemsetAsync(d_buf.get() + n_bytes, 0, (size_t) (padded - n_bytes), st));
        DN_TRY(hipMemcpyAsync(d_err, &no_error, sizeof(no_error), hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));

        hipLaunchKernelGGL(k_count_newlines, dim3(grid_capped(n_tiles)), dim3(kNT), 0, st, (const uint4 *) d_buf.get(), n_tiles, d_tile_count.get());
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanNT), 0, st, d_tile_count.get(), n_tiles, d_tile_off.get(), d_total.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&n_newlines, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (n_newlines < 0 || n_newlines > n_bytes) return dn::fail(DN_E_STATE, "dn_gtf_scan: newline count out of range");

        const int64_t n_starts = n_newlines + 1;                       // the last one starts an empty line when the bytes end in '\n'
        const int64_t n_blocks = (n_starts + kNT - 1) / kNT;
        DN_TRY(d_line_start.alloc(sizeof(int64_t) * (size_t) n_starts));
        DN_TRY(d_keep.alloc((size_t) n_starts));
        DN_TRY(d_block_kept.alloc(sizeof(int32_t) * (size_t) n_blocks));
        DN_TRY(d_block_off.alloc(sizeof(int64_t) * (size_t) n_blocks));
        DN_TRY(rec.alloc(n_starts));
        DN_TRY(hipMemsetAsync(d_line_start, 0, sizeof(int64_t), st));
        hipLaunchKernelGGL(k_line_starts, dim3(grid_capped(n_tiles)), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_tiles,
                           (const int64_t *) d_tile_off.get(), d_line_start.get(), n_starts);
        hipLaunchKernelGGL(k_parse_lines, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_bytes,
                           (const int64_t *) d_line_start.get(), n_starts, rec.view(), d_keep.get(), d_block_kept.get(), d_err.get());
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanNT), 0, st, d_block_kept.get(), n_blocks, d_block_off.get(), d_total.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&kept, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(&first_error, d_err, sizeof(first_error), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));

        *n_lines = n_newlines + (buf[n_bytes - 1] != '\n' ? 1 : 0);
        if (first_error != no_error) {
            *err_line = (int64_t) (first_error >> 8);
            *err_kind = (int32_t) (first_error & 0xffu);
            DN_TRY(hipEventRecord(e2, st));
        } else {
            if (kept < 0 || kept > row_cap) return dn::fail(DN_E_INVALID, "dn_gtf_scan: more exon lines than the caller's tables hold");
            DN_TRY(row.alloc(kept));
            if (kept > 0) {
                hipLaunchKernelGGL(k_compact, dim3((unsigned) n_blocks), dim3(kNT), 0, st, n_starts, (const uint8_t *) d_keep.get(),
                                   (const int64_t *) d_block_off.get(), rec.view(), row.view(), kept);
                DN_TRY(hipGetLastError());
            }
            DN_TRY(hipEventRecord(e2, st));
#define GTF_OUT(h, d, T) do { if (kept > 0) DN_TRY(hipMemcpyAsync(h, d, sizeof(T) * (size_t) kept, hipMemcpyDeviceToHost, st)); } while (0)
            GTF_OUT(line, row.line, int64_t); GTF_OUT(chr_beg, row.chr_beg, int64_t); GTF_OUT(chr_len, row.chr_len, int32_t);
            GTF_OUT(chr_hash, row.chr_hash, uint64_t); GTF_OUT(start, row.start, int64_t); GTF_OUT(end, row.end, int64_t);
            GTF_OUT(gene_beg, row.gene_beg, int64_t); GTF_OUT(gene_len, row.gene_len, int32_t); GTF_OUT(gene_hash, row.gene_hash, uint64_t);
#undef GTF_OUT
            *n_rows = kept;
        }
        DN_TRY(hipStreamSynchronize(st));
        if (copy_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *copy_ms = ms; }
        if (device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *device_ms = ms; }
        return DN_OK;
    });
}

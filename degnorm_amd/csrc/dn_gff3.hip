// dn_gff3.hip -- GFF3 annotation scan on the device (Gff3AnnotationLoader, loaders.gff3_scan; include/degnorm_amd.h, "GFF3
// annotation scan", defines the rule and dn_gff3.hpp holds it, one source for both builds).
//
// In GFF3 an exon line may name only its Parent, and the gene's name stands on a line any distance away, before or behind:
// the gene of an exon comes out of a join over the whole file.  So the file's text stays on the device for one load (a
// handle owns one buffer of the file's size, padded to whole tiles and zeroed), and windows that end at line ends are
// uploaded to their place in it.  Per window:
//   1  k_count_newlines, k_scan, k_line_starts   where every line starts (LineTable, dn_lines.hpp, shared with dn_gtf.hip and
//                      dn_sam.hip), over the tiles the window touches; the lines of the first tile that belong to the
//                      window before are not looked at again
//   2  k_gff3_parse    one lane per line: exon row, node row, ##FASTA or nothing (gff3::parse_line), FNV-1a hashes of the
//                      spans; the first faulty line and the first ##FASTA line by atomicMin
//   3  k_gff3_mark     exon lines and node lines above the ##FASTA line, counted per 256-line block
//   4  k_scan twice, k_compact twice (dn_annot.hpp, the exon table shared with dn_gtf.hip): exon rows to a table that goes
//                      to the host, node rows to the end of the handle's node store, which has no line, start and end
//                      columns; both in file order, all offsets global to the file
// dn_gff3_resolve then sorts the node rows as (ID hash, ordinal) with hipcub::DeviceRadixSort::SortPairs -- a stable sort, so
// nodes of one hash stay in file order -- and runs one lane per exon that named a Parent (k_gff3_walk, gff3::walk): a
// lower-bound search on the hash, a scan of the run of that hash for the first node whose ID has the wanted bytes, at most
// eight such lookups.  Nothing is decided by a hash alone.
// Every text byte is read through Bytes at positions below its line's end, which is at most the bytes uploaded; the spans
// the walk reads were cut out of lines by k_gff3_parse, and those the caller hands to dn_gff3_resolve are checked against
// the bytes uploaded before they reach the device.  dn_gff3_scan_host runs the same text line after line on the caller's bytes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <numeric>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_annot.hpp"
#include "dn_gff3.hpp"

namespace {

namespace g3 = dn::gff3;

constexpr int64_t kMaxWindow = (int64_t) 1 << 30;

// Lane j takes line n_head + j of the tile range: the lines before belong to the window before.  Positions are relative to
// the first tile, which starts at byte `base` of the file; line numbers count from line_base.
__global__ __launch_bounds__(kNT) void k_gff3_parse(const uint8_t *__restrict__ buf, int64_t base, int64_t rel_end,
                                                     const int64_t *__restrict__ line_start, int64_t n_starts, int64_t n_head, int64_t line_base,
                                                     uint64_t mask, ExonCols rec, uint8_t *__restrict__ kind,
                                                     unsigned long long *__restrict__ first_error, unsigned long long *__restrict__ first_fasta)
{
    const int64_t j = (int64_t) blockIdx.x * kNT + threadIdx.x, i = n_head + j;
    if (i >= n_starts) return;
    int64_t beg, end;
    line_span(line_start, n_starts, rel_end, i, &beg, &end);
    const int64_t line = line_base + j + 1;
    Bytes b(buf);
    g3::Line L{0, 0, 0, 0, 0, 0, 0};
    const int r = beg >= 0 && beg <= end && end <= rel_end ? g3::parse_line(b, beg, end, L) : dn::kSkip;
    if (r < 0) report_error(first_error, line, -r);
    if (r == g3::kFasta) atomicMin(first_fasta, (unsigned long long) line);
    const bool row = r == dn::kExon || r == g3::kNode;
    if (row) {
        const uint64_t c_hash = dn::fnv1a(b, L.c_lo, L.c_hi), a_hash = dn::fnv1a(b, L.a_lo, L.a_hi);
        rec.line[j] = line;
        rec.c_beg[j] = base + L.c_lo;
        rec.c_len[j] = (int32_t) (L.c_hi - L.c_lo);
        rec.c_hash[j] = r == g3::kNode ? c_hash & mask : c_hash;
        rec.start[j] = L.start;
        rec.end[j] = L.end;
        rec.a_beg[j] = base + L.a_lo;
        rec.a_len[j] = (int32_t) (L.a_hi - L.a_lo);
        rec.a_hash[j] = L.open ? a_hash & mask : a_hash;
        rec.open[j] = (uint8_t) L.open;
    }
    kind[j] = (uint8_t) (row ? r : 0);
}

__global__ __launch_bounds__(kNT) void k_gff3_mark(const uint8_t *__restrict__ kind, int64_t n_lanes, int64_t line_base,
                                                    const unsigned long long *__restrict__ first_fasta, int32_t *__restrict__ block_exons,
                                                    int32_t *__restrict__ block_nodes)
{
    const int64_t j = (int64_t) blockIdx.x * kNT + threadIdx.x;
    const unsigned long long fasta = *first_fasta;
    int total;
    (void) block_exclusive(kept_as(dn::kExon, kind, j, n_lanes, line_base, fasta) ? 1 : 0, &total);
    if (threadIdx.x == 0) block_exons[blockIdx.x] = total;
    (void) block_exclusive(kept_as(g3::kNode, kind, j, n_lanes, line_base, fasta) ? 1 : 0, &total);
    if (threadIdx.x == 0) block_nodes[blockIdx.x] = total;
}

__global__ __launch_bounds__(kNT) void k_gff3_iota(uint32_t *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (i < n) out[i] = (uint32_t) i;
}

// one lane per exon that named a Parent: its gene's name span and hash, or the first link error by atomicMin
__global__ __launch_bounds__(kNT) void k_gff3_walk(const uint8_t *__restrict__ buf, g3::Nodes N, int64_t n, const int64_t *__restrict__ line,
                                                    const int64_t *__restrict__ par_beg, const int32_t *__restrict__ par_len,
                                                    const uint64_t *__restrict__ par_hash, int64_t *__restrict__ name_beg,
                                                    int32_t *__restrict__ name_len, uint64_t *__restrict__ name_hash,
                                                    unsigned long long *__restrict__ first_error)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (i >= n) return;
    Bytes want(buf), have(buf);
    int64_t beg = par_beg[i];
    int32_t len = par_len[i];
    uint64_t hash = par_hash[i];
    const int e = g3::walk(want, have, N, &beg, &len, &hash);
    if (e) {
        report_error(first_error, line[i], e);
        beg = 0; len = 0; hash = 0;
    }
    name_beg[i] = beg;
    name_len[i] = len;
    name_hash[i] = hash;
}

// the node rows of the file so far, in file order: c = the ID (hash masked), a = the name or the Parent
struct NodeStore {
    dn::GrowBuffer<int64_t> id_beg, a_beg;
    dn::GrowBuffer<int32_t> id_len, a_len;
    dn::GrowBuffer<uint64_t> id_hash, a_hash;
    dn::GrowBuffer<uint8_t> open;
    hipError_t reserve(int64_t need, int64_t used, hipStream_t st)
    {
        hipError_t e = id_beg.reserve(need, used, st);
        if (e == hipSuccess) e = a_beg.reserve(need, used, st);
        if (e == hipSuccess) e = id_len.reserve(need, used, st);
        if (e == hipSuccess) e = a_len.reserve(need, used, st);
        if (e == hipSuccess) e = id_hash.reserve(need, used, st);
        if (e == hipSuccess) e = a_hash.reserve(need, used, st);
        if (e == hipSuccess) e = open.reserve(need, used, st);
        return e;
    }
    ExonCols at(int64_t k) const
    {
        return ExonCols{nullptr, id_beg.get() + k, nullptr, nullptr, a_beg.get() + k, id_len.get() + k, a_len.get() + k, id_hash.get() + k,
                    a_hash.get() + k, open.get() + k};
    }
};

}  // namespace

struct dn_gff3_ {
    int device = 0;
    int64_t total = 0, padded = 0;
    uint64_t mask = ~0ull;
    dn::Stream st;
    dn::DeviceBuffer<uint8_t> buf;
    int64_t pos = 0;             // bytes uploaded so far
    int64_t tail_nl = 0;         // '\n' among them from the start of the tile that holds byte `pos` on
    int64_t lines = 0;           // lines so far
    int64_t n_nodes = 0;
    bool open_line = false;      // the bytes so far do not end in '\n': nothing may follow
    bool ended = false;          // a window held ##FASTA
    NodeStore nodes;
};

extern "C" int dn_gff3_open(int device, int64_t total_bytes, int32_t hash_bits, dn_gff3 *out)
{
    dn::clear_error();
    if (!out || total_bytes < 1 || hash_bits < 1 || hash_bits > 64) return dn::fail(DN_E_INVALID, "dn_gff3_open: bad argument");
    *out = nullptr;
    DN_TRY(hipSetDevice(device));
    const int64_t padded = (total_bytes + kTile - 1) / kTile * kTile;
    // the text, about 45 bytes a node line and 110 bytes a line of one window; annotation lines are longer than that
    size_t free_b = 0, total_b = 0;
    DN_TRY(hipMemGetInfo(&free_b, &total_b));
    const double need = (double) padded * 1.5 + (double) (64 << 20);
    if (need > (double) free_b)
        return dn::fail(DN_E_INVALID, "dn_gff3_open: a file of " + std::to_string(total_bytes) + " bytes needs about " + std::to_string((int64_t) (need / 1048576.0))
                        + " MiB of device memory to stay resident, and " + std::to_string((int64_t) (free_b >> 20)) + " MiB are free");
    dn_gff3_ *h = new (std::nothrow) dn_gff3_();
    if (!h) return dn::fail(DN_E_INVALID, "dn_gff3_open: out of host memory");
    h->device = device; h->total = total_bytes; h->padded = padded; h->mask = g3::hash_mask(hash_bits);
    const int rc = [&]() -> int {
        DN_TRY(h->st.create(hipStreamCreate));
        DN_TRY(h->buf.alloc((size_t) padded));
        DN_TRY(hipMemsetAsync(h->buf, 0, (size_t) padded, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    }();
    if (rc != DN_OK) { delete h; return rc; }
    *out = h;
    return DN_OK;
}

extern "C" int dn_gff3_close(dn_gff3 h)
{
    if (!h) return DN_OK;
    (void) hipSetDevice(h->device);
    if (h->st) (void) hipStreamSynchronize(h->st);
    delete h;
    return DN_OK;
}

// dn_gff3_window, and with `strand` not null dn_gff3_window_strand: field seven of every exon row of the window
static int gff3_window(dn_gff3 h, const uint8_t *bytes, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                       int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                       int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *pending, uint8_t *strand, int64_t *fasta_line,
                       int64_t *err_line, int32_t *err_kind, double *copy_ms, double *device_ms)
{
    dn::clear_error();
    if (!h || !bytes || n_bytes < 1 || n_bytes > kMaxWindow || row_cap < 0 || !n_lines || !n_rows || !line || !chr_beg || !chr_len || !chr_hash
        || !start || !end || !gene_beg || !gene_len || !gene_hash || !pending || !fasta_line || !err_line || !err_kind)
        return dn::fail(DN_E_INVALID, "dn_gff3_window: bad argument");
    *n_lines = 0; *n_rows = 0; *fasta_line = 0; *err_line = 0; *err_kind = 0;
    if (n_bytes > h->total - h->pos) return dn::fail(DN_E_INVALID, "dn_gff3_window: more bytes than the handle was opened for");
    if (h->open_line) return dn::fail(DN_E_STATE, "dn_gff3_window: the window before did not end at a line end");
    if (h->ended) return dn::fail(DN_E_STATE, "dn_gff3_window: a window before held ##FASTA, which ends the annotation");
    const int64_t t0 = h->pos / kTile, t1 = (h->pos + n_bytes + kTile - 1) / kTile, n_tiles = t1 - t0, base = t0 * kTile;
    const int64_t head = h->pos - base, rel_end = head + n_bytes, n_head = h->tail_nl, line_base = h->lines;
    // what the stream reads or writes: owned here, so that it outlives the wait of dn::synced
    dn::Event e0, e1, e2;
    dn::DeviceBuffer<uint8_t> d_kind, d_strand;
    dn::DeviceBuffer<int32_t> d_block_exons, d_block_nodes;
    dn::DeviceBuffer<int64_t> d_exon_off, d_node_off;
    dn::DeviceBuffer<unsigned long long> d_marks;                   // first error, first ##FASTA line
    LineTable lines;
    ExonBuffers rec, row;
    const unsigned long long none[2] = {kNoError, kNoFasta};
    unsigned long long marks[2] = {kNoError, kNoFasta};
    int64_t n_exons = 0, n_new_nodes = 0;
    DN_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st;
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(e2.create(hipEventCreate));
        DN_TRY(lines.alloc(n_tiles));
        DN_TRY(d_marks.alloc(sizeof(none)));
        DN_TRY(hipEventRecord(e0, st));
        DN_TRY(hipMemcpyAsync(h->buf.get() + h->pos, bytes, (size_t) n_bytes, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_marks, none, sizeof(none), hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));

        const uint8_t *tiles = h->buf.get() + base;                 // the tiles the window touches; behind rel_end they hold zeros
        const int rc = lines.find(st, tiles, n_tiles, n_head, rel_end, "dn_gff3_window");
        if (rc != DN_OK) return rc;
        const int64_t n_newlines = lines.n_newlines, n_starts = lines.n_starts;
        const int64_t n_lanes = n_starts - n_head;
        const int64_t n_blocks = (n_lanes + kNT - 1) / kNT;
        DN_TRY(d_kind.alloc((size_t) n_lanes));
        DN_TRY(d_block_exons.alloc(sizeof(int32_t) * (size_t) n_blocks));
        DN_TRY(d_block_nodes.alloc(sizeof(int32_t) * (size_t) n_blocks));
        DN_TRY(d_exon_off.alloc(sizeof(int64_t) * (size_t) n_blocks));
        DN_TRY(d_node_off.alloc(sizeof(int64_t) * (size_t) n_blocks));
        DN_TRY(rec.alloc(n_lanes, true));
        hipLaunchKernelGGL(k_gff3_parse, dim3((unsigned) n_blocks), dim3(kNT), 0, st, tiles, base, rel_end, (const int64_t *) lines.line_start.get(),
                           n_starts, n_head, line_base, h->mask, rec.view(), d_kind.get(), d_marks.get(), d_marks.get() + 1);
        if (strand)
            hipLaunchKernelGGL(k_strand_check, dim3((unsigned) n_blocks), dim3(kNT), 0, st, tiles, rel_end, (const int64_t *) lines.line_start.get(),
                               n_starts, n_head, line_base, (const uint8_t *) d_kind.get(), (int) DN_GFF3_E_STRAND, d_marks.get());
        hipLaunchKernelGGL(k_gff3_mark, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (const uint8_t *) d_kind.get(), n_lanes, line_base,
                           (const unsigned long long *) d_marks.get() + 1, d_block_exons.get(), d_block_nodes.get());
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanNT), 0, st, d_block_exons.get(), n_blocks, d_exon_off.get(), lines.total.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&n_exons, lines.total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanNT), 0, st, d_block_nodes.get(), n_blocks, d_node_off.get(), lines.total.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&n_new_nodes, lines.total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(marks, d_marks, sizeof(marks), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));

        const int64_t win_lines = n_newlines - n_head + (bytes[n_bytes - 1] != '\n' ? 1 : 0);
        const bool fasta = marks[1] != kNoFasta;
        int64_t e_line = 0;
        int32_t e_kind = 0;
        const bool error = unpack_error(marks[0], &e_line, &e_kind) && (!fasta || (unsigned long long) e_line < marks[1]);
        *n_lines = win_lines;
        if (fasta) *fasta_line = (int64_t) marks[1];
        if (error) {
            *err_line = e_line;
            *err_kind = e_kind;
            DN_TRY(hipEventRecord(e2, st));
        } else {
            if (n_exons < 0 || n_exons > n_lanes || n_new_nodes < 0 || n_new_nodes > n_lanes) return dn::fail(DN_E_STATE, "dn_gff3_window: row counts out of range");
            if (n_exons > row_cap) return dn::fail(DN_E_INVALID, "dn_gff3_window: more exon lines than the caller's tables hold");
            if (h->n_nodes + n_new_nodes > 0x7fffffffll) return dn::fail(DN_E_INVALID, "dn_gff3_window: more than 2^31 - 1 lines with an ID");
            DN_TRY(row.alloc(n_exons, true));
            DN_TRY(h->nodes.reserve(h->n_nodes + n_new_nodes, h->n_nodes, st));
            if (n_exons > 0)
                hipLaunchKernelGGL(k_compact, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (int) dn::kExon, (const uint8_t *) d_kind.get(), n_lanes,
                                   line_base, (const unsigned long long *) d_marks.get() + 1, (const int64_t *) d_exon_off.get(), rec.view(), row.view(),
                                   n_exons);
            if (n_new_nodes > 0)
                hipLaunchKernelGGL(k_compact, dim3((unsigned) n_blocks), dim3(kNT), 0, st, (int) g3::kNode, (const uint8_t *) d_kind.get(), n_lanes,
                                   line_base, (const unsigned long long *) d_marks.get() + 1, (const int64_t *) d_node_off.get(), rec.view(),
                                   h->nodes.at(h->n_nodes), n_new_nodes);
            DN_TRY(hipGetLastError());
            if (strand && n_exons > 0) {                            // the text is resident: c_beg is an offset into the file
                DN_TRY(d_strand.alloc((size_t) n_exons));
                hipLaunchKernelGGL(k_row_strand, dim3((unsigned) ((n_exons + kNT - 1) / kNT)), dim3(kNT), 0, st, (const uint8_t *) h->buf.get(),
                                   h->pos + n_bytes, (const int64_t *) row.c_beg.get(), n_exons, d_strand.get());
                DN_TRY(hipGetLastError());
            }
            DN_TRY(hipEventRecord(e2, st));
            if (strand && n_exons > 0) DN_TRY(hipMemcpyAsync(strand, d_strand, (size_t) n_exons, hipMemcpyDeviceToHost, st));
            DN_TRY(copy_rows(st, ExonCols{line, chr_beg, start, end, gene_beg, chr_len, gene_len, chr_hash, gene_hash, pending}, row.view(), n_exons));
        }
        DN_TRY(hipStreamSynchronize(st));
        if (copy_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *copy_ms = ms; }
        if (device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *device_ms = ms; }
        if (!error) {
            // the handle moves on only when the window's rows are the caller's
            const int64_t new_pos = h->pos + n_bytes, tile = new_pos / kTile * kTile;
            h->tail_nl = tile > h->pos ? count_newlines(bytes + (tile - h->pos), new_pos - tile) : h->tail_nl + (n_newlines - n_head);
            h->pos = new_pos;
            h->lines += win_lines;
            h->n_nodes += n_new_nodes;
            h->open_line = bytes[n_bytes - 1] != '\n';
            h->ended = fasta;
            *n_rows = n_exons;
        }
        return DN_OK;
    });
}

extern "C" int dn_gff3_window(dn_gff3 h, const uint8_t *bytes, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                              int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                              int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *pending, int64_t *fasta_line,
                              int64_t *err_line, int32_t *err_kind, double *copy_ms, double *device_ms)
{
    return gff3_window(h, bytes, n_bytes, row_cap, n_lines, n_rows, line, chr_beg, chr_len, chr_hash, start, end, gene_beg, gene_len, gene_hash,
                       pending, nullptr, fasta_line, err_line, err_kind, copy_ms, device_ms);
}

extern "C" int dn_gff3_window_strand(dn_gff3 h, const uint8_t *bytes, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                                     int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                                     int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *pending, uint8_t *strand,
                                     int64_t *fasta_line, int64_t *err_line, int32_t *err_kind, double *copy_ms, double *device_ms)
{
    return gff3_window(h, bytes, n_bytes, row_cap, n_lines, n_rows, line, chr_beg, chr_len, chr_hash, start, end, gene_beg, gene_len, gene_hash,
                       pending, strand, fasta_line, err_line, err_kind, copy_ms, device_ms);
}

extern "C" int dn_gff3_resolve(dn_gff3 h, int64_t n, const int64_t *line, const int64_t *par_beg, const int32_t *par_len, const uint64_t *par_hash,
                               int64_t *name_beg, int32_t *name_len, uint64_t *name_hash, int64_t *n_nodes, int64_t *err_line, int32_t *err_kind,
                               double *resolve_ms)
{
    dn::clear_error();
    if (!h || n < 0 || !n_nodes || !err_line || !err_kind || (n > 0 && (!line || !par_beg || !par_len || !par_hash || !name_beg || !name_len || !name_hash)))
        return dn::fail(DN_E_INVALID, "dn_gff3_resolve: bad argument");
    *n_nodes = h->n_nodes; *err_line = 0; *err_kind = 0;
    if (resolve_ms) *resolve_ms = 0.0;
    for (int64_t k = 0; k < n; k++)                                 // the device reads these spans
        if (line[k] < 1 || par_len[k] < 0 || par_beg[k] < 0 || par_beg[k] > h->pos || (int64_t) par_len[k] > h->pos - par_beg[k])
            return dn::fail(DN_E_INVALID, "dn_gff3_resolve: a parent span outside the bytes uploaded");
    if (n == 0) return DN_OK;
    const int64_t m = h->n_nodes;
    const size_t m1 = (size_t) (m > 0 ? m : 1);
    dn::Event e1, e2;
    dn::DeviceBuffer<uint64_t> d_key, d_par_hash, d_name_hash;
    dn::DeviceBuffer<uint32_t> d_iota, d_ord;
    dn::DeviceBuffer<int64_t> d_line, d_par_beg, d_name_beg;
    dn::DeviceBuffer<int32_t> d_par_len, d_name_len;
    dn::DeviceBuffer<unsigned long long> d_err;
    dn::Scratch scratch;
    unsigned long long first_error = kNoError;
    DN_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st;
    return dn::synced(st, [&]() -> int {
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(e2.create(hipEventCreate));
        DN_TRY(d_key.alloc(sizeof(uint64_t) * m1));
        DN_TRY(d_iota.alloc(sizeof(uint32_t) * m1));
        DN_TRY(d_ord.alloc(sizeof(uint32_t) * m1));
        DN_TRY(d_line.alloc(sizeof(int64_t) * (size_t) n));
        DN_TRY(d_par_beg.alloc(sizeof(int64_t) * (size_t) n));
        DN_TRY(d_par_len.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(d_par_hash.alloc(sizeof(uint64_t) * (size_t) n));
        DN_TRY(d_name_beg.alloc(sizeof(int64_t) * (size_t) n));
        DN_TRY(d_name_len.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(d_name_hash.alloc(sizeof(uint64_t) * (size_t) n));
        DN_TRY(d_err.alloc(sizeof(unsigned long long)));
        DN_TRY(hipMemcpyAsync(d_line, line, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_par_beg, par_beg, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_par_len, par_len, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_par_hash, par_hash, sizeof(uint64_t) * (size_t) n, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_err, &kNoError, sizeof(kNoError), hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));
        if (m > 0) {
            hipLaunchKernelGGL(k_gff3_iota, dim3((unsigned) ((m + kNT - 1) / kNT)), dim3(kNT), 0, st, d_iota.get(), m);
            DN_TRY(hipGetLastError());
            DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
                return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint64_t *) h->nodes.id_hash.get(), d_key.get(), (const uint32_t *) d_iota.get(),
                                                          d_ord.get(), (int) m, 0, 64, st);
            }));
        }
        const g3::Nodes N{m, d_key.get(), d_ord.get(), h->nodes.id_beg.get(), h->nodes.id_len.get(), h->nodes.a_beg.get(), h->nodes.a_len.get(),
                          h->nodes.a_hash.get(), h->nodes.open.get()};
        hipLaunchKernelGGL(k_gff3_walk, dim3((unsigned) ((n + kNT - 1) / kNT)), dim3(kNT), 0, st, (const uint8_t *) h->buf.get(), N, n,
                           (const int64_t *) d_line.get(), (const int64_t *) d_par_beg.get(), (const int32_t *) d_par_len.get(),
                           (const uint64_t *) d_par_hash.get(), d_name_beg.get(), d_name_len.get(), d_name_hash.get(), d_err.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(e2, st));
        DN_TRY(hipMemcpyAsync(&first_error, d_err, sizeof(first_error), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(name_beg, d_name_beg, sizeof(int64_t) * (size_t) n, hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(name_len, d_name_len, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(name_hash, d_name_hash, sizeof(uint64_t) * (size_t) n, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        (void) unpack_error(first_error, err_line, err_kind);
        if (resolve_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *resolve_ms = ms; }
        return DN_OK;
    });
}

// dn_gff3_scan_host, and with `strand` not null dn_gff3_scan_host_strand
static int gff3_scan_host(const uint8_t *data, int64_t n_bytes, int32_t hash_bits, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                          int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                          int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *strand, int64_t *n_nodes, int64_t *n_walked,
                          int64_t *err_line, int32_t *err_kind)
{
    dn::clear_error();
    if (!data || n_bytes < 1 || hash_bits < 1 || hash_bits > 64 || row_cap < 0 || !n_lines || !n_rows || !line || !chr_beg || !chr_len || !chr_hash
        || !start || !end || !gene_beg || !gene_len || !gene_hash || !n_nodes || !n_walked || !err_line || !err_kind)
        return dn::fail(DN_E_INVALID, "dn_gff3_scan_host: bad argument");
    *n_lines = 0; *n_rows = 0; *n_nodes = 0; *n_walked = 0; *err_line = 0; *err_kind = 0;
    const uint64_t mask = g3::hash_mask(hash_bits);
    dn::HostText in{data}, other{data};
    struct Exon { int64_t line, c_beg, start, end, a_beg; int32_t c_len, a_len; int open; };
    std::vector<Exon> exons;
    std::vector<int64_t> id_beg, a_beg;
    std::vector<int32_t> id_len, a_len;
    std::vector<uint64_t> id_hash, a_hash;
    std::vector<uint8_t> open;
    int64_t lines = 0;
    bool ended = false;
    *n_lines = count_newlines(data, n_bytes) + (data[n_bytes - 1] != '\n' ? 1 : 0);
    for (int64_t pos = 0; pos < n_bytes; lines++) {
        const uint8_t *nl = (const uint8_t *) memchr(data + pos, '\n', (size_t) (n_bytes - pos));
        const int64_t stop = nl ? (int64_t) (nl - data) : n_bytes;
        if (!ended) {
            g3::Line L{0, 0, 0, 0, 0, 0, 0};
            const int r = g3::parse_line(in, pos, stop, L);
            if (r < 0) {
                *err_line = lines + 1;
                *err_kind = -r;
                return DN_OK;
            }
            if (r == g3::kFasta) ended = true;
            if (r == dn::kExon && strand && !dn::strand_field(in, pos, stop)) {
                *err_line = lines + 1;
                *err_kind = DN_GFF3_E_STRAND;
                return DN_OK;
            }
            if (r == dn::kExon)
                exons.push_back(Exon{lines + 1, L.c_lo, L.start, L.end, L.a_lo, (int32_t) (L.c_hi - L.c_lo), (int32_t) (L.a_hi - L.a_lo), L.open});
            if (r == g3::kNode) {
                id_beg.push_back(L.c_lo); id_len.push_back((int32_t) (L.c_hi - L.c_lo)); id_hash.push_back(dn::fnv1a(in, L.c_lo, L.c_hi) & mask);
                const uint64_t hh = dn::fnv1a(in, L.a_lo, L.a_hi);
                a_beg.push_back(L.a_lo); a_len.push_back((int32_t) (L.a_hi - L.a_lo)); a_hash.push_back(L.open ? hh & mask : hh);
                open.push_back((uint8_t) L.open);
            }
        }
        pos = stop + 1;
    }
    const int64_t m = (int64_t) id_beg.size();
    if (m > 0x7fffffffll) return dn::fail(DN_E_INVALID, "dn_gff3_scan_host: more than 2^31 - 1 lines with an ID");
    if ((int64_t) exons.size() > row_cap) return dn::fail(DN_E_INVALID, "dn_gff3_scan_host: more exon lines than the caller's tables hold");
    std::vector<uint32_t> ord((size_t) m);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return id_hash[x] < id_hash[y]; });
    std::vector<uint64_t> key((size_t) m);
    for (int64_t k = 0; k < m; k++) key[(size_t) k] = id_hash[ord[(size_t) k]];
    const g3::Nodes N{m, key.data(), ord.data(), id_beg.data(), id_len.data(), a_beg.data(), a_len.data(), a_hash.data(), open.data()};
    *n_nodes = m;
    int64_t walked = 0;
    for (size_t k = 0; k < exons.size(); k++) {
        const Exon &x = exons[k];
        int64_t g_beg = x.a_beg;
        int32_t g_len = x.a_len;
        uint64_t g_hash = dn::fnv1a(in, x.a_beg, x.a_beg + x.a_len);
        if (x.open) {
            g_hash &= mask;
            walked++;
            const int e = g3::walk(in, other, N, &g_beg, &g_len, &g_hash);
            if (e) {
                *err_line = x.line;
                *err_kind = e;
                *n_walked = walked;
                return DN_OK;
            }
        }
        line[k] = x.line; chr_beg[k] = x.c_beg; chr_len[k] = x.c_len; chr_hash[k] = dn::fnv1a(in, x.c_beg, x.c_beg + x.c_len);
        start[k] = x.start; end[k] = x.end; gene_beg[k] = g_beg; gene_len[k] = g_len; gene_hash[k] = g_hash;
        if (strand) strand[k] = dn::strand_field(in, x.c_beg, n_bytes);
    }
    *n_rows = (int64_t) exons.size();
    *n_walked = walked;
    return DN_OK;
}

extern "C" int dn_gff3_scan_host(const uint8_t *data, int64_t n_bytes, int32_t hash_bits, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                                 int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                                 int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, int64_t *n_nodes, int64_t *n_walked, int64_t *err_line,
                                 int32_t *err_kind)
{
    return gff3_scan_host(data, n_bytes, hash_bits, row_cap, n_lines, n_rows, line, chr_beg, chr_len, chr_hash, start, end, gene_beg, gene_len,
                          gene_hash, nullptr, n_nodes, n_walked, err_line, err_kind);
}

extern "C" int dn_gff3_scan_host_strand(const uint8_t *data, int64_t n_bytes, int32_t hash_bits, int64_t row_cap, int64_t *n_lines,
                                        int64_t *n_rows, int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start,
                                        int64_t *end, int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *strand,
                                        int64_t *n_nodes, int64_t *n_walked, int64_t *err_line, int32_t *err_kind)
{
    if (!strand) return dn::fail(DN_E_INVALID, "dn_gff3_scan_host_strand: bad argument");
    return gff3_scan_host(data, n_bytes, hash_bits, row_cap, n_lines, n_rows, line, chr_beg, chr_len, chr_hash, start, end, gene_beg, gene_len,
                          gene_hash, strand, n_nodes, n_walked, err_line, err_kind);
}

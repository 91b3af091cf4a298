// dn_sam.hip -- SAM alignment lines -> BAM records on the device (bam.sam_records, bam.sam_to_bam; include/degnorm_amd.h,
// "SAM text to BAM records", defines the encoding and dn_sam.hpp holds it, one source for both builds).
//
// A window of alignment lines that ends at a line end goes to the GPU and comes back as the record stream, in input order:
//   1  k_count_newlines, k_scan, k_line_starts   where every line starts (LineTable, dn_lines.hpp, shared with dn_gtf.hip and
//                      dn_gff3.hip)
//   2  k_sam_measure   one lane per line: every field checked, the record's size and its number of float payloads; the
//                      first faulty line in file order by atomicMin (report_error, dn_lines.hpp)
//   3  hipcub::DeviceScan::ExclusiveSum of the sizes -> the record offsets, and of the payload counts -> the first patch
//                      entry of every line; both over n_lines + 1 entries, so the last one is the total
//   4  k_sam_emit      one lane per line: the record to its offset, byte by byte with ordinary vector stores, and the
//                      line's patch entries
// The host then fills the float payloads: the text a patch entry points at goes through strtod and the four bytes go to the
// stream.  The device never reads a decimal, and both builds write the same bytes.
// Every text byte is read through Bytes at positions below the line's end, which is at most n_bytes; every store of a
// record lies inside the size its line measured (sam::Writer), and the stream is allocated with the sum of those sizes.
// dn_sam_encode_host runs the same two walks line after line on the caller's bytes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_lines.hpp"
#include "dn_sam.hpp"

namespace {

using dn::sam::LineSize;
using dn::sam::Refs;

constexpr int64_t kMaxWindow = (int64_t) 1 << 30;

// size[i], n_float[i] for i < n_lines, and 0 in entry n_lines, which makes the exclusive sums end with the totals
__global__ __launch_bounds__(kNT) void k_sam_measure(const uint8_t *__restrict__ buf, int64_t n_bytes, const int64_t *__restrict__ line_start,
                                                      int64_t n_starts, int64_t n_lines, Refs R, int64_t *__restrict__ size,
                                                      int64_t *__restrict__ n_float, unsigned long long *__restrict__ first_error)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (i > n_lines) return;
    LineSize L{0, 0};
    if (i < n_lines) {
        int64_t beg, end;
        line_span(line_start, n_starts, n_bytes, i, &beg, &end);
        Bytes b(buf);
        const int e = beg <= end && end <= n_bytes ? dn::sam::encode_line<Bytes, false>(b, beg, end, R, nullptr, 0, 0, nullptr, 0, L) : DN_SAM_E_EMPTY;
        if (e) {
            report_error(first_error, i + 1, e);
            L.size = 0; L.n_float = 0;
        }
    }
    size[i] = L.size;
    n_float[i] = L.n_float;
}

__global__ __launch_bounds__(kNT) void k_sam_emit(const uint8_t *__restrict__ buf, int64_t n_bytes, const int64_t *__restrict__ line_start,
                                                   int64_t n_starts, int64_t n_lines, Refs R, const int64_t *__restrict__ rec_off,
                                                   const int64_t *__restrict__ patch_off, uint8_t *__restrict__ out, int64_t n_out,
                                                   int64_t *__restrict__ patch, int64_t n_patch)
{
    const int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (i >= n_lines) return;
    int64_t beg, end;
    line_span(line_start, n_starts, n_bytes, i, &beg, &end);
    const int64_t o = rec_off[i], cap = rec_off[i + 1] - o, f = patch_off[i], fcap = patch_off[i + 1] - f;
    if (beg > end || end > n_bytes || o < 0 || cap < 0 || o + cap > n_out || f < 0 || fcap < 0 || f + fcap > n_patch) return;
    Bytes b(buf);
    LineSize L;
    (void) dn::sam::encode_line<Bytes, true>(b, beg, end, R, out + o, cap, o, patch + 2 * f, fcap, L);
}

// the references of a call: what the entry points check before any work
int check_refs(const char *who, int32_t n_ref, const uint64_t *hash, const int32_t *id, const int64_t *beg, const int32_t *len,
               const uint8_t *names, int64_t n_names)
{
    if (n_ref < 0 || n_names < 0 || (n_ref > 0 && (!hash || !id || !beg || !len)) || (n_names > 0 && !names))
        return dn::fail(DN_E_INVALID, std::string(who) + ": bad argument");
    for (int32_t k = 0; k < n_ref; k++) {
        if (len[k] < 0 || beg[k] < 0 || beg[k] > n_names || len[k] > n_names - beg[k])
            return dn::fail(DN_E_INVALID, std::string(who) + ": a reference name outside the names");
        if (k > 0 && hash[k] < hash[k - 1]) return dn::fail(DN_E_INVALID, std::string(who) + ": the reference table is not sorted by hash");
    }
    return DN_OK;
}

// the float payloads: the text of entry k -- up to ',', a tab, the line end or the end of the bytes -- through strtod
void fill_floats(const uint8_t *text, int64_t n_bytes, uint8_t *out, const int64_t *patch, int64_t n_patch)
{
    std::string tok;
    for (int64_t k = 0; k < n_patch; k++) {
        const int64_t at = patch[2 * k], lo = patch[2 * k + 1];
        int64_t hi = lo;
        while (hi < n_bytes && text[hi] != ',' && text[hi] != '\t' && text[hi] != '\r' && text[hi] != '\n') hi++;
        tok.assign((const char *) text + lo, (size_t) (hi - lo));
        const float v = (float) strtod(tok.c_str(), nullptr);
        memcpy(out + at, &v, sizeof(v));
    }
}

int check_call(const char *who, const uint8_t *text, int64_t n_bytes, uint8_t *out, int64_t out_cap, int64_t *rec_off, int64_t rec_cap,
               int64_t *patch, int64_t patch_cap, int64_t *n_lines, int64_t *n_rec, int64_t *n_out, int64_t *n_patch, int64_t *err_line,
               int32_t *err_kind)
{
    if (!text || n_bytes < 1 || n_bytes > kMaxWindow || out_cap < 0 || rec_cap < 1 || patch_cap < 0 || (out_cap > 0 && !out) || !rec_off
        || (patch_cap > 0 && !patch) || !n_lines || !n_rec || !n_out || !n_patch || !err_line || !err_kind)
        return dn::fail(DN_E_INVALID, std::string(who) + ": bad argument");
    *n_lines = 0; *n_rec = 0; *n_out = 0; *n_patch = 0; *err_line = 0; *err_kind = 0;
    return DN_OK;
}

int capacity_error(const char *who, int64_t n_lines, int64_t rec_cap, int64_t total, int64_t out_cap, int64_t floats, int64_t patch_cap)
{
    if (n_lines + 1 > rec_cap || total > out_cap || floats > patch_cap)
        return dn::fail(DN_E_INVALID, std::string(who) + ": " + std::to_string(n_lines) + " records of " + std::to_string(total) + " bytes with "
                        + std::to_string(floats) + " float payloads do not fit the caller's arrays");
    return DN_OK;
}

}  // namespace

extern "C" int dn_sam_encode_host(const uint8_t *text, int64_t n_bytes, int32_t n_ref, const uint64_t *ref_hash, const int32_t *ref_id,
                                  const int64_t *ref_name_beg, const int32_t *ref_name_len, const uint8_t *names, int64_t n_names,
                                  uint8_t *out, int64_t out_cap, int64_t *rec_off, int64_t rec_cap, int64_t *patch, int64_t patch_cap,
                                  int64_t *n_lines, int64_t *n_rec, int64_t *n_out, int64_t *n_patch, int64_t *err_line, int32_t *err_kind)
{
    dn::clear_error();
    int rc = check_call("dn_sam_encode_host", text, n_bytes, out, out_cap, rec_off, rec_cap, patch, patch_cap, n_lines, n_rec, n_out, n_patch,
                        err_line, err_kind);
    if (rc == DN_OK) rc = check_refs("dn_sam_encode_host", n_ref, ref_hash, ref_id, ref_name_beg, ref_name_len, names, n_names);
    if (rc != DN_OK) return rc;
    const Refs R{n_ref, ref_hash, ref_id, ref_name_beg, ref_name_len, names};
    const int64_t lines = count_newlines(text, n_bytes) + (text[n_bytes - 1] != '\n' ? 1 : 0);
    *n_lines = lines;
    // where the lines start, then the measure pass
    std::vector<int64_t> start((size_t) lines + 1), off((size_t) lines + 1), foff((size_t) lines + 1);
    int64_t pos = 0;
    for (int64_t i = 0; i < lines; i++) {
        start[(size_t) i] = pos;
        const uint8_t *nl = (const uint8_t *) memchr(text + pos, '\n', (size_t) (n_bytes - pos));
        pos = nl ? (int64_t) (nl - text) + 1 : n_bytes + 1;
    }
    start[(size_t) lines] = pos;                                // one behind the '\n' of the last line, or n_bytes + 1 without one
    dn::HostText in{text};
    int64_t total = 0, n_float = 0;
    for (int64_t i = 0; i < lines; i++) {
        LineSize L;
        const int e = dn::sam::encode_line<dn::HostText, false>(in, start[(size_t) i], start[(size_t) i + 1] - 1, R, nullptr, 0, 0, nullptr, 0, L);
        if (e) {
            *err_line = i + 1;
            *err_kind = e;
            return DN_OK;
        }
        off[(size_t) i] = total;
        foff[(size_t) i] = n_float;
        total += L.size;
        n_float += L.n_float;
    }
    off[(size_t) lines] = total;
    foff[(size_t) lines] = n_float;
    rc = capacity_error("dn_sam_encode_host", lines, rec_cap, total, out_cap, n_float, patch_cap);
    if (rc != DN_OK) return rc;
    for (int64_t i = 0; i < lines; i++) {
        LineSize L;
        const int64_t o = off[(size_t) i], f = foff[(size_t) i];
        (void) dn::sam::encode_line<dn::HostText, true>(in, start[(size_t) i], start[(size_t) i + 1] - 1, R, out + o, off[(size_t) i + 1] - o, o,
                                                             patch ? patch + 2 * f : nullptr, foff[(size_t) i + 1] - f, L);
    }
    memcpy(rec_off, off.data(), sizeof(int64_t) * (size_t) (lines + 1));
    fill_floats(text, n_bytes, out, patch, n_float);
    *n_rec = lines; *n_out = total; *n_patch = n_float;
    return DN_OK;
}

extern "C" int dn_sam_encode(int device, const uint8_t *text, int64_t n_bytes, int32_t n_ref, const uint64_t *ref_hash, const int32_t *ref_id,
                             const int64_t *ref_name_beg, const int32_t *ref_name_len, const uint8_t *names, int64_t n_names, uint8_t *out,
                             int64_t out_cap, int64_t *rec_off, int64_t rec_cap, int64_t *patch, int64_t patch_cap, int64_t *n_lines,
                             int64_t *n_rec, int64_t *n_out, int64_t *n_patch, int64_t *err_line, int32_t *err_kind, double *copy_ms,
                             double *device_ms)
{
    dn::clear_error();
    int rc = check_call("dn_sam_encode", text, n_bytes, out, out_cap, rec_off, rec_cap, patch, patch_cap, n_lines, n_rec, n_out, n_patch,
                        err_line, err_kind);
    if (rc == DN_OK) rc = check_refs("dn_sam_encode", n_ref, ref_hash, ref_id, ref_name_beg, ref_name_len, names, n_names);
    if (rc != DN_OK) return rc;
    const int64_t n_tiles = (n_bytes + kTile - 1) / kTile, padded = n_tiles * kTile;
    const size_t n_tab = (size_t) (n_ref > 0 ? n_ref : 1);
    // what the stream reads or writes: owned here, so that it outlives the wait of dn::synced
    dn::Stream st;
    dn::Event e0, e1, e2;
    dn::DeviceBuffer<uint8_t> d_buf, d_names, d_out;
    dn::DeviceBuffer<int32_t> d_ref_id, d_ref_len;
    dn::DeviceBuffer<uint64_t> d_ref_hash;
    dn::DeviceBuffer<int64_t> d_ref_beg, d_size, d_float, d_rec_off, d_patch_off, d_patch;
    dn::DeviceBuffer<unsigned long long> d_err;
    LineTable table;
    dn::Scratch scratch;
    unsigned long long first_error = kNoError;
    int64_t total = 0, floats = 0;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(e2.create(hipEventCreate));
        DN_TRY(d_buf.alloc((size_t) padded));
        DN_TRY(table.alloc(n_tiles));
        DN_TRY(d_err.alloc(sizeof(unsigned long long)));
        DN_TRY(d_ref_hash.alloc(sizeof(uint64_t) * n_tab));
        DN_TRY(d_ref_id.alloc(sizeof(int32_t) * n_tab));
        DN_TRY(d_ref_beg.alloc(sizeof(int64_t) * n_tab));
        DN_TRY(d_ref_len.alloc(sizeof(int32_t) * n_tab));
        DN_TRY(d_names.alloc((size_t) (n_names > 0 ? n_names : 1)));
        DN_TRY(hipEventRecord(e0, st));
        DN_TRY(upload_padded(st, d_buf, text, n_bytes, padded));
        DN_TRY(hipMemcpyAsync(d_err, &kNoError, sizeof(kNoError), hipMemcpyHostToDevice, st));
        if (n_ref > 0) {
            DN_TRY(hipMemcpyAsync(d_ref_hash, ref_hash, sizeof(uint64_t) * (size_t) n_ref, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_ref_id, ref_id, sizeof(int32_t) * (size_t) n_ref, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_ref_beg, ref_name_beg, sizeof(int64_t) * (size_t) n_ref, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_ref_len, ref_name_len, sizeof(int32_t) * (size_t) n_ref, hipMemcpyHostToDevice, st));
        }
        if (n_names > 0) DN_TRY(hipMemcpyAsync(d_names, names, (size_t) n_names, hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));

        const int find_rc = table.find(st, d_buf, n_tiles, 0, n_bytes, "dn_sam_encode");
        if (find_rc != DN_OK) return find_rc;
        const int64_t n_starts = table.n_starts;
        const int64_t lines = table.n_newlines + (text[n_bytes - 1] != '\n' ? 1 : 0);
        const size_t n_per_line = sizeof(int64_t) * (size_t) (lines + 1);
        const unsigned n_blocks = (unsigned) ((lines + 1 + kNT - 1) / kNT);
        const Refs R{n_ref, d_ref_hash.get(), d_ref_id.get(), d_ref_beg.get(), d_ref_len.get(), d_names.get()};
        *n_lines = lines;
        DN_TRY(d_size.alloc(n_per_line));
        DN_TRY(d_float.alloc(n_per_line));
        DN_TRY(d_rec_off.alloc(n_per_line));
        DN_TRY(d_patch_off.alloc(n_per_line));
        hipLaunchKernelGGL(k_sam_measure, dim3(n_blocks), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_bytes,
                           (const int64_t *) table.line_start.get(), n_starts, lines, R, d_size.get(), d_float.get(), d_err.get());
        DN_TRY(hipGetLastError());
        DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const int64_t *) d_size.get(), d_rec_off.get(), (int) (lines + 1), st);
        }));
        DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const int64_t *) d_float.get(), d_patch_off.get(), (int) (lines + 1), st);
        }));
        DN_TRY(hipMemcpyAsync(&first_error, d_err, sizeof(first_error), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(&total, d_rec_off.get() + lines, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(&floats, d_patch_off.get() + lines, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));

        if (unpack_error(first_error, err_line, err_kind)) {
            DN_TRY(hipEventRecord(e2, st));
        } else {
            if (total < 0 || floats < 0) return dn::fail(DN_E_STATE, "dn_sam_encode: sizes out of range");
            const int cap_rc = capacity_error("dn_sam_encode", lines, rec_cap, total, out_cap, floats, patch_cap);
            if (cap_rc != DN_OK) return cap_rc;
            DN_TRY(d_out.alloc((size_t) (total > 0 ? total : 1)));
            DN_TRY(d_patch.alloc(sizeof(int64_t) * 2 * (size_t) (floats > 0 ? floats : 1)));
            if (lines > 0) {
                hipLaunchKernelGGL(k_sam_emit, dim3((unsigned) ((lines + kNT - 1) / kNT)), dim3(kNT), 0, st, (const uint8_t *) d_buf.get(), n_bytes,
                                   (const int64_t *) table.line_start.get(), n_starts, lines, R, (const int64_t *) d_rec_off.get(),
                                   (const int64_t *) d_patch_off.get(), d_out.get(), total, d_patch.get(), floats);
                DN_TRY(hipGetLastError());
            }
            DN_TRY(hipEventRecord(e2, st));
            if (total > 0) DN_TRY(hipMemcpyAsync(out, d_out, (size_t) total, hipMemcpyDeviceToHost, st));
            DN_TRY(hipMemcpyAsync(rec_off, d_rec_off, n_per_line, hipMemcpyDeviceToHost, st));
            if (floats > 0) DN_TRY(hipMemcpyAsync(patch, d_patch, sizeof(int64_t) * 2 * (size_t) floats, hipMemcpyDeviceToHost, st));
        }
        DN_TRY(hipStreamSynchronize(st));
        if (first_error == kNoError) {
            for (int64_t k = 0; k < floats; k++)           // the device wrote these: hold them to the arrays before they are used
                if (patch[2 * k] < 0 || patch[2 * k] + 4 > total || patch[2 * k + 1] < 0 || patch[2 * k + 1] >= n_bytes)
                    return dn::fail(DN_E_STATE, "dn_sam_encode: patch entry out of range");
            fill_floats(text, n_bytes, out, patch, floats);
            *n_rec = lines; *n_out = total; *n_patch = floats;
        }
        if (copy_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *copy_ms = ms; }
        if (device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *device_ms = ms; }
        return DN_OK;
    });
}

// dn_sort.hip -- coordinate sort of the records of a BAM file whose whole inflated record stream is resident on the device.
//
//   inflate   the BGZF blocks go up a window at a time and every block is inflated to its place in one buffer of the size of
//             the stream (dn::inflate_launch, InflateBlock::dst_off), so the buffer is the file's record stream, contiguous
//   frame     dn::frame_window (tid = -1) over the buffer in pieces; a record that a piece cuts starts the next piece
//   keys      k_sort_keys, one lane per record: block_size, refID and pos give the key and the record's length, and the
//             record is checked (sort_record, on the record view of dn_bam_record.hpp).  The first error in input order
//             wins (dn::note_error)
//   sort      hipcub::DeviceRadixSort::SortPairs of (key, ordinal), which is stable, over the bits that can differ: those of
//             the largest pos + 1 met, then those of n_ref -- two LSD passes over one ping-pong pair of arrays
//   scan      the lengths in sorted order, exclusive sum: where each record goes
//   gather    k_sort_gather, 16 lanes per record (four records a wavefront; a record is a few hundred bytes): the output is
//             written in 16-byte pieces aligned to the destination; the 16 source bytes of a piece come from two aligned
//             16-byte loads and a funnel shift by the record's source misalignment.  The at most 15 bytes before the first
//             and behind the last aligned piece share their 16 bytes with the neighbouring records and are copied byte by byte
//   deflate   (dn_bam_sort_deflate, for a caller that writes the file with the library's encoder) ranges of the sorted stream
//             become BGZF blocks where the stream lies (dn::deflate_device); the unsorted copy, dead by then, lends the slots
//
// The order: ascending key = dn::ref_key(refID) << 32 | (uint32) (pos + 1): refID -1 has the largest ref_key, so unplaced
// records go last, and pos -1 sorts first within a reference; records of equal key keep their order in the input.
// (The arrays hold n_ref in place of that largest value: the same order in fewer bits.)
//
// The per-record steps (sort_record, copy_plan, load16_at) are __host__ __device__ functions; the host build runs them in
// plain loops on bytes the caller inflated, with std::stable_sort in place of the radix sort, so the sorted stream is
// testable without a device.
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
#include "dn_inflate.hpp"
#include "dn_frame.hpp"
#include "dn_deflate.hpp"
#include "dn_bam_record.hpp"

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kGroup = 16;                         // lanes that copy one record
constexpr int64_t kSlack = 64;                     // bytes behind the stream: load16_at reads whole aligned 16-byte pieces
constexpr int64_t kPieceDefault = (int64_t) 256 << 20;
constexpr int64_t kGridCap = 1 << 20;

enum { kSortOk = 0, kSortShape = 1, kSortRef = 2, kSortPos = 3 };

// The record at byte o of the stream s: its key, its length with the block_size field and pos + 1; kSortOk or what is wrong
// with it.  The framing established that the record lies inside the stream; the bounds are checked again so that offsets
// that do not belong to s cannot lead outside.
DN_HD int sort_record(const uint8_t *s, int64_t n_bytes, int64_t o, int32_t n_ref, uint64_t &key, uint32_t &len, uint32_t &pos1)
{
    key = 0; len = 0; pos1 = 0;
    dn::BamHead H;
    if (!dn::bam_head(s, n_bytes, o, H) || !H.names_fit()) return kSortShape;
    len = (uint32_t) (4 + H.bs);
    if (H.ref < -1 || H.ref >= n_ref) return kSortRef;
    if (H.pos < -1) return kSortPos;
    pos1 = (uint32_t) (H.pos + 1);
    const uint32_t rk = dn::ref_key(H.ref);                 // the arrays hold n_ref in place of kUnplaced
    key = (uint64_t) (rk == dn::kUnplaced ? (uint32_t) n_ref : rk) << 32 | pos1;
    return kSortOk;
}

// How the len bytes that go to out[d ..) are written: `head` single bytes up to the next multiple of 16, n_body aligned
// pieces of 16 bytes, `tail` single bytes.
struct CopyPlan {
    int32_t head, tail;
    int64_t n_body;
};

DN_HD CopyPlan copy_plan(int64_t d, int64_t len)
{
    int64_t head = (16 - (d & 15)) & 15;
    if (head > len) head = len;
    return CopyPlan{(int32_t) head, (int32_t) ((len - head) & 15), (len - head) >> 4};
}

DN_HD void ld16(const uint8_t *p, uint32_t *w)
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
    memcpy(w, p, 16);
#endif
}

DN_HD void st16(uint8_t *p, const uint32_t *w)
{
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
#else
    memcpy(p, w, 16);
#endif
}

DN_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t bits) { return (uint32_t) (((uint64_t) hi << 32 | lo) >> bits); }

// The 16 bytes s[sp .. sp + 16) from the two aligned 16-byte pieces that hold them (s is 16-byte aligned and has kSlack
// bytes behind its last one).  Which four of the eight words, and the shift inside them, depend on sp & 15 alone.
DN_HD void load16_at(const uint8_t *s, int64_t sp, uint32_t *o)
{
    const int64_t sa = sp & ~(int64_t) 15;
    const uint32_t sh = (uint32_t) (sp & 15), r = (sh & 3) * 8;
    uint32_t w[8];
    ld16(s + sa, w);
    ld16(s + sa + 16, w + 4);
    switch (sh >> 2) {
    case 0: o[0] = funnel(w[0], w[1], r); o[1] = funnel(w[1], w[2], r); o[2] = funnel(w[2], w[3], r); o[3] = funnel(w[3], w[4], r); break;
    case 1: o[0] = funnel(w[1], w[2], r); o[1] = funnel(w[2], w[3], r); o[2] = funnel(w[3], w[4], r); o[3] = funnel(w[4], w[5], r); break;
    case 2: o[0] = funnel(w[2], w[3], r); o[1] = funnel(w[3], w[4], r); o[2] = funnel(w[4], w[5], r); o[3] = funnel(w[5], w[6], r); break;
    default: o[0] = funnel(w[3], w[4], r); o[1] = funnel(w[4], w[5], r); o[2] = funnel(w[5], w[6], r); o[3] = funnel(w[6], w[7], r); break;
    }
}

// Piece c of the plan P of the record copied from in[src ..) to out[d ..): c < 0 stands for the single bytes (c = -1 - k,
// k < 32: byte k of the head for k < 16, byte k - 16 of the tail otherwise)
DN_HD void copy_piece(const uint8_t *in, uint8_t *out, int64_t src, int64_t d, int64_t len, const CopyPlan &P, int64_t c)
{
    if (c >= 0) {
        uint32_t o[4];
        load16_at(in, src + P.head + 16 * c, o);
        st16(out + d + P.head + 16 * c, o);
        return;
    }
    const int32_t k = (int32_t) (-1 - c);
    if (k < 16) {
        if (k < P.head) out[d + k] = in[src + k];
    } else if (k - 16 < P.tail) {
        const int64_t t = len - P.tail + (k - 16);
        out[d + t] = in[src + t];
    }
}

// offsets of a piece's records (relative to the piece, which starts at byte `base`) -> the file's tables, from record `first`
__global__ __launch_bounds__(kNT) void k_sort_keys(const uint8_t *__restrict__ s, int64_t n_bytes, const int64_t *__restrict__ piece_off,
                                                   int64_t base, int64_t n, int64_t first, int32_t n_ref, int64_t *__restrict__ off,
                                                   uint64_t *__restrict__ key, uint32_t *__restrict__ ord, uint32_t *__restrict__ len,
                                                   unsigned long long *__restrict__ err)
{
    uint32_t top = 0;
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) {
        const int64_t o = piece_off[i] + base;
        uint64_t k;
        uint32_t l, p1;
        const int e = sort_record(s, n_bytes, o, n_ref, k, l, p1);
        off[first + i] = o; key[first + i] = k; ord[first + i] = (uint32_t) (first + i); len[first + i] = l;
        if (e != kSortOk) dn::note_error(err, first + i, e);
        top = p1 > top ? p1 : top;
    }
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const uint32_t other = (uint32_t) __shfl_xor((int) top, m);
        top = other > top ? other : top;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && top > 0) atomicMax(err + 1, (unsigned long long) top);
}

// the lengths in sorted order, and a zero behind them: their exclusive sum then ends with the size of the stream
__global__ __launch_bounds__(kNT) void k_sort_lengths(const uint32_t *__restrict__ ord, const uint32_t *__restrict__ len, int64_t n,
                                                      int64_t *__restrict__ slen)
{
    for (int64_t j = (int64_t) blockIdx.x * kNT + threadIdx.x; j <= n; j += (int64_t) gridDim.x * kNT) slen[j] = j < n ? (int64_t) len[ord[j]] : 0;
}

// kGroup lanes per record of the output
__global__ __launch_bounds__(kNT) void k_sort_gather(const uint8_t *__restrict__ in, const int64_t *__restrict__ off, const uint32_t *__restrict__ ord,
                                                     const int64_t *__restrict__ dst, int64_t n, uint8_t *__restrict__ out)
{
    const int lane = threadIdx.x & (kGroup - 1);
    for (int64_t j = (int64_t) blockIdx.x * (kNT / kGroup) + threadIdx.x / kGroup; j < n; j += (int64_t) gridDim.x * (kNT / kGroup)) {
        const int64_t src = off[ord[j]], d = dst[j], len = dst[j + 1] - d;
        const CopyPlan P = copy_plan(d, len);
        for (int k = lane; k < 32; k += kGroup) copy_piece(in, out, src, d, len, P, -1 - k);
        for (int64_t c = lane; c < P.n_body; c += kGroup) copy_piece(in, out, src, d, len, P, c);
    }
}

inline int bits_of(uint64_t v)
{
    int b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

}  // namespace

struct dn_bam_sort_s {
    int device = -1;                   // < 0: the host build
    int32_t n_ref = 0;
    int64_t n_bytes = 0, segment = 0, piece = kPieceDefault;
    int64_t filled = 0, n_records = 0, n_windows = 0, n_fixups = 0;
    bool failed = false, finished = false;
    double frame_ms = 0.0;
    // the host build
    std::vector<uint8_t> h_in, h_out;
    std::vector<int64_t> h_dst;
    // the device path
    dn::Stream st;
    dn::DeviceBuffer<uint8_t> in, out;
    dn::InflateWindow ingest;          // of dn_bam_sort_window; armed by dn_bam_sort_expect_crc
    dn::GrowBuffer<int64_t> piece_off, off, dst;
    dn::GrowBuffer<uint64_t> key, key2;
    dn::GrowBuffer<uint32_t> ord, ord2, len;
    dn::DeviceBuffer<unsigned long long> err;      // [0] the first error, [1] the largest pos + 1
    dn::FrameWork frame;
    dn::Scratch scratch;
    dn::Event ev0, ev1, ev2, ev3;
    // dn_bam_sort_deflate on the device: its tables, and its own region where the dead input copy is too small for one block
    dn::DeflateTables deflate;
    dn::DeviceBuffer<uint8_t> deflate_region;
    bool deflating = false;
};

namespace {

int record_error(dn_bam_sort h, int code, int64_t idx, int32_t ref, int32_t pos)
{
    const std::string who = dn::record_name(idx, ref, pos);
    h->failed = true;
    switch (code) {
    case kSortShape: return dn::record_shape_error(who);
    case kSortRef: return dn::record_reference_error(who, h->n_ref);
    default: return dn::fail(DN_E_INVALID, who + " has a position below -1");
    }
}

int bad_size_error(dn_bam_sort h, int64_t idx, int64_t at, int32_t bs)
{
    h->failed = true;
    return dn::fail(DN_E_INVALID, "malformed BAM record " + std::to_string(idx) + " at byte " + std::to_string(at) + " of the record stream: block_size " +
                                  std::to_string(bs) + " is below 32");
}

int cut_error(dn_bam_sort h, int64_t left)
{
    h->failed = true;
    return dn::record_cut_error(h->n_records, left);
}

// the steps of dn_bam_sort_finish on the host's copy of the stream
struct HostSort {
    dn_bam_sort h;
    std::vector<int64_t> piece_off, off;
    std::vector<uint64_t> key;
    std::vector<uint32_t> ord, len;
    unsigned long long err = dn::kNoError;

    // frame the piece [base, base + n): nr records, `used` bytes; bad: the record behind them has the block_size bad_bs
    int frame(int64_t base, int64_t n, int64_t &nr, int64_t &used, bool &bad, int32_t &bad_bs)
    {
        const uint8_t *w = h->h_in.data() + base;
        piece_off.resize((size_t) (n / 36 + 2));
        int64_t fix = 0;
        nr = used = 0;
        const int rc = dn_bam_frame_segments_host(w, n, -1, nullptr, h->segment, piece_off.data(), (int64_t) piece_off.size(), &nr, &used, &fix);
        h->n_fixups += fix;
        if (rc == DN_OK) return DN_OK;
        // the only record the framing of a mixed stream refuses is one with a block_size below 32: the serial walk finds it
        nr = used = 0;
        while (used + 4 <= n) {
            const int32_t bs = (int32_t) dn::le32(w + used);
            if (bs < dn::kBamMinSize) { bad = true; bad_bs = bs; dn::clear_error(); return DN_OK; }
            if (used + 4 + (int64_t) bs > n) break;
            piece_off[(size_t) nr++] = used;
            used += 4 + (int64_t) bs;
        }
        return rc;
    }
    int keys(int64_t base, int64_t nr, uint32_t &top)
    {
        const size_t first = (size_t) h->n_records;
        off.resize(first + (size_t) nr); key.resize(off.size()); ord.resize(off.size()); len.resize(off.size());
        for (int64_t i = 0; i < nr; i++) {
            const size_t g = first + (size_t) i;
            uint32_t p1;
            off[g] = piece_off[(size_t) i] + base;
            const int e = sort_record(h->h_in.data(), h->n_bytes, off[g], h->n_ref, key[g], len[g], p1);
            ord[g] = (uint32_t) g;
            if (e != kSortOk) dn::note_error(&err, (int64_t) g, e);
            top = p1 > top ? p1 : top;
        }
        return DN_OK;
    }
    int first_error(unsigned long long &e, int32_t &ref, int32_t &pos)
    {
        e = err;
        if (e != dn::kNoError) dn::error_record_host(off.data(), dn::error_ordinal(e), h->h_in.data(), h->n_bytes, ref, pos);
        return DN_OK;
    }
    int sort_and_gather(int /*pos_bits*/, int /*ref_bits*/, int64_t &total)
    {
        const int64_t n = h->n_records;
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        h->h_dst.assign((size_t) n + 1, 0);
        for (int64_t j = 0; j < n; j++) h->h_dst[(size_t) j + 1] = h->h_dst[(size_t) j] + len[ord[(size_t) j]];
        total = h->h_dst[(size_t) n];
        if (total != h->n_bytes) return DN_OK;
        h->h_out.assign((size_t) (h->n_bytes + kSlack), 0);
        for (int64_t j = 0; j < n; j++) {
            const int64_t src = off[ord[(size_t) j]], d = h->h_dst[(size_t) j], l = h->h_dst[(size_t) j + 1] - d;
            const CopyPlan P = copy_plan(d, l);
            for (int64_t c = -32; c < P.n_body; c++) copy_piece(h->h_in.data(), h->h_out.data(), src, d, l, P, c);
        }
        return DN_OK;
    }
};

// the same on the device; what queued copies write lives in this object, which dn_bam_sort_finish declares outside the
// body it hands to dn::synced
struct DeviceSort {
    dn_bam_sort h;
    unsigned long long h_err[2] = {dn::kNoError, 0};
    int64_t h_total = 0;
    dn::ErrorProbe probe;
    float sort_ms = 0.f, gather_ms = 0.f;

    int frame(int64_t base, int64_t n, int64_t &nr, int64_t &used, bool &bad, int32_t &bad_bs)
    {
        dn::FrameResult R;
        const int rc = dn::frame_window(h->st, h->frame, h->in.get() + base, n, -1, nullptr, h->segment, -1, h->piece_off, R);
        h->n_fixups += R.n_fixups;
        h->frame_ms += R.device_ms;
        nr = R.n_rec; used = R.consumed;
        if (rc != DN_OK && R.bad) { bad = true; bad_bs = R.bad_bs; dn::clear_error(); return DN_OK; }
        return rc;
    }
    int keys(int64_t base, int64_t nr, uint32_t &)
    {
        hipStream_t st = h->st;
        const int64_t first = h->n_records;
        if (first + nr > (int64_t) INT32_MAX) return dn::fail(DN_E_INVALID, "dn_bam_sort_finish: more than 2^31 - 1 records");
        DN_TRY(h->off.reserve(first + nr, first, st)); DN_TRY(h->key.reserve(first + nr, first, st));
        DN_TRY(h->ord.reserve(first + nr, first, st)); DN_TRY(h->len.reserve(first + nr, first, st));
        DN_TRY(hipEventRecord(h->ev0, st));
        hipLaunchKernelGGL(k_sort_keys, dim3(dn::grid_for(nr, kNT, kGridCap)), dim3(kNT), 0, st, (const uint8_t *) h->in.get(), h->n_bytes,
                           (const int64_t *) h->piece_off.get(), base, nr, first, h->n_ref, h->off.get(), h->key.get(), h->ord.get(), h->len.get(),
                           h->err.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(h->ev1, st));
        DN_TRY(hipStreamSynchronize(st));
        float ms = 0.f;
        DN_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        sort_ms += ms;
        return DN_OK;
    }
    int first_error(unsigned long long &e, int32_t &ref, int32_t &pos)
    {
        hipStream_t st = h->st;
        DN_TRY(hipMemcpyAsync(h_err, h->err, sizeof(h_err), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        e = h_err[0];
        return e == dn::kNoError ? DN_OK : dn::error_record_device(st, h->off, dn::error_ordinal(e), h->in, h->n_bytes, probe, ref, pos);
    }
    uint32_t top() const { return (uint32_t) h_err[1]; }
    int sort_and_gather(int pos_bits, int ref_bits, int64_t &total)
    {
        hipStream_t st = h->st;
        const int64_t n = h->n_records;
        DN_TRY(h->key2.reserve(n, 0, st)); DN_TRY(h->ord2.reserve(n, 0, st)); DN_TRY(h->dst.reserve(n + 1, 0, st));
        uint64_t *ka = h->key.get(), *kb = h->key2.get();
        uint32_t *oa = h->ord.get(), *ob = h->ord2.get();
        DN_TRY(hipEventRecord(h->ev0, st));
        const int range[2][2] = {{0, pos_bits}, {32, 32 + ref_bits}};
        for (int pass = 0; pass < 2 && n > 1; pass++) {
            if (range[pass][0] == range[pass][1]) continue;
            DN_TRY(h->scratch.run([&](void *tmp, size_t &bytes) {
                return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, kb, oa, ob, (int) n, range[pass][0], range[pass][1], st);
            }));
            std::swap(ka, kb);
            std::swap(oa, ob);
        }
        hipLaunchKernelGGL(k_sort_lengths, dim3(dn::grid_for(n + 1, kNT, kGridCap)), dim3(kNT), 0, st, (const uint32_t *) oa, (const uint32_t *) h->len.get(), n,
                           h->dst.get());
        DN_TRY(hipGetLastError());
        DN_TRY(h->scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, h->dst.get(), h->dst.get(), (int) (n + 1), st);
        }));
        DN_TRY(hipEventRecord(h->ev1, st));
        DN_TRY(hipMemcpyAsync(&h_total, h->dst + n, sizeof(h_total), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        float ms = 0.f;
        DN_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        sort_ms += ms;
        total = h_total;
        if (total != h->n_bytes) return DN_OK;                         // the records do not tile the stream: nothing is copied
        DN_TRY(hipEventRecord(h->ev2, st));
        hipLaunchKernelGGL(k_sort_gather, dim3(dn::grid_for(n, kNT / kGroup, kGridCap)), dim3(kNT), 0, st, (const uint8_t *) h->in.get(), (const int64_t *) h->off.get(),
                           (const uint32_t *) oa, (const int64_t *) h->dst.get(), n, h->out.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(h->ev3, st));
        DN_TRY(hipStreamSynchronize(st));
        DN_TRY(hipEventElapsedTime(&gather_ms, h->ev2, h->ev3));
        return DN_OK;
    }
};

// Frame the stream in pieces, build the tables, sort and gather; the first error in input order is the one reported.
template <class B> int run_sort(dn_bam_sort h, B &be, uint32_t &top)
{
    int64_t base = 0, piece = h->piece;
    while (base < h->n_bytes) {
        const int64_t n = std::min(piece, h->n_bytes - base);
        int64_t nr = 0, used = 0;
        bool bad = false;
        int32_t bad_bs = 0;
        int rc = be.frame(base, n, nr, used, bad, bad_bs);
        if (rc != DN_OK) { h->failed = true; return rc; }
        if (nr > 0) {
            if ((rc = be.keys(base, nr, top)) != DN_OK) { h->failed = true; return rc; }
            unsigned long long e = dn::kNoError;
            int32_t ref = -1, pos = -1;
            if ((rc = be.first_error(e, ref, pos)) != DN_OK) { h->failed = true; return rc; }
            if (e != dn::kNoError) return record_error(h, dn::error_code(e), dn::error_ordinal(e), ref, pos);
        }
        if (bad) return bad_size_error(h, h->n_records + nr, base + used, bad_bs);
        h->n_records += nr;
        if (used == 0) {                                                // the piece holds no whole record
            if (n == h->n_bytes - base) return cut_error(h, n);
            if (piece > INT32_MAX / 2) { h->failed = true; return dn::fail(DN_E_INVALID, "record " + std::to_string(h->n_records) + " is longer than 2^30 bytes"); }
            piece *= 2;
            continue;
        }
        base += used;
    }
    return DN_OK;
}

}  // namespace

extern "C" int dn_bam_sort_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes)
{
    dn::clear_error();
    if (device < 0 || !free_bytes || !total_bytes) return dn::fail(DN_E_INVALID, "dn_bam_sort_device_memory: bad argument");
    size_t f = 0, t = 0;
    DN_TRY(hipSetDevice(device));
    DN_TRY(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t) f;
    *total_bytes = (int64_t) t;
    return DN_OK;
}

extern "C" int dn_bam_sort_create(int device, int32_t n_ref, int64_t n_inflated, int64_t segment_bytes, int64_t piece_bytes, dn_bam_sort *out)
{
    dn::clear_error();
    if (!out || n_ref < 0 || n_inflated < 0 || piece_bytes < 0 || (segment_bytes != 0 && segment_bytes < dn::kFrameSegmentMin))
        return dn::fail(DN_E_INVALID, "dn_bam_sort_create: bad argument (segment_bytes is 0 or at least 64)");
    dn_bam_sort h = new dn_bam_sort_s();
    h->device = device < 0 ? -1 : device;
    h->n_ref = n_ref;
    h->n_bytes = n_inflated;
    h->segment = segment_bytes;
    h->piece = piece_bytes == 0 ? kPieceDefault : std::min<int64_t>(std::max<int64_t>(piece_bytes, 64), (int64_t) 1 << 30);
    const int rc = [&]() -> int {
        if (device < 0) {
            try {
                h->h_in.assign((size_t) (n_inflated + kSlack), 0);
            } catch (const std::bad_alloc &) {
                return dn::fail(DN_E_INVALID, "dn_bam_sort_create: no host memory for " + std::to_string(n_inflated) + " bytes of records");
            }
            return DN_OK;
        }
        DN_TRY(hipSetDevice(device));
        DN_TRY(h->st.create(hipStreamCreate));
        DN_TRY(h->in.alloc((size_t) (n_inflated + kSlack)));
        DN_TRY(h->out.alloc((size_t) (n_inflated + kSlack)));
        DN_TRY(dn::alloc_padded(h->err, 2));
        DN_TRY(hipMemsetAsync(h->in.get() + n_inflated, 0, (size_t) kSlack, h->st));
        DN_TRY(hipMemsetAsync(h->err, 0xff, sizeof(unsigned long long), h->st));
        DN_TRY(hipMemsetAsync(h->err + 1, 0, sizeof(unsigned long long), h->st));
        DN_TRY(h->ev0.create(hipEventCreate)); DN_TRY(h->ev1.create(hipEventCreate));
        DN_TRY(h->ev2.create(hipEventCreate)); DN_TRY(h->ev3.create(hipEventCreate));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    }();
    if (rc != DN_OK) { delete h; return rc; }
    *out = h;
    return DN_OK;
}

extern "C" void dn_bam_sort_destroy(dn_bam_sort h)
{
    if (!h) return;
    if (h->device >= 0) {
        (void) hipSetDevice(h->device);
        if (h->st) (void) hipStreamSynchronize(h->st);
    }
    delete h;
}

extern "C" int dn_bam_sort_expect_crc(dn_bam_sort h, const uint32_t *crc32, int64_t n_blocks)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_sort_expect_crc: bad argument");
    if (h->device < 0) return dn::fail(DN_E_STATE, "dn_bam_sort_expect_crc: a host sort is handed inflated bytes; its caller checks them");
    return h->ingest.arm("dn_bam_sort_expect_crc", crc32, n_blocks);
}

extern "C" int dn_bam_sort_window(dn_bam_sort h, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                                  const int32_t *isize, int32_t head_skip, int32_t *status, double *inflate_ms)
{
    dn::clear_error();
    if (h) h->ingest.take();
    int rc = dn::check_handle(h, "dn_bam_sort_window", "sort", true);
    if (rc != DN_OK) return rc;
    if (n_comp < 0 || (n_comp > 0 && !comp) || n_blocks < 0 || n_blocks > INT32_MAX || (n_blocks > 0 && (!pay_off || !pay_len || !isize || !status)) ||
        head_skip < 0)
        return dn::fail(DN_E_INVALID, "dn_bam_sort_window: bad argument");
    int64_t at = 0;
    rc = h->ingest.plan("dn_bam_sort_window", "dn_bam_sort_expect_crc", n_comp, n_blocks, pay_off, pay_len, isize, head_skip, -1, h->filled, at);
    if (rc != DN_OK) return rc;
    if (at > h->n_bytes) return dn::fail(DN_E_INVALID, "dn_bam_sort_window: the blocks hold more bytes than dn_bam_sort_create was told");
    hipStream_t st = h->st;
    DN_TRY(hipSetDevice(h->device));
    if (inflate_ms) *inflate_ms = 0.0;
    return dn::synced(st, [&]() -> int {
        bool ok = true;
        const int wrc = h->ingest.run(st, comp, n_comp, h->in, status, inflate_ms, ok);
        if (wrc != DN_OK) return wrc;
        if (!ok) { h->failed = true; return DN_OK; }
        h->filled = at;
        h->n_windows++;
        return DN_OK;
    });
}

extern "C" int dn_bam_sort_window_host(dn_bam_sort h, const uint8_t *data, int64_t n_data, int32_t head_skip)
{
    dn::clear_error();
    const int rc = dn::check_handle(h, "dn_bam_sort_window_host", "sort", false);
    if (rc != DN_OK) return rc;
    if (n_data < 0 || (n_data > 0 && !data) || head_skip < 0) return dn::fail(DN_E_INVALID, "dn_bam_sort_window_host: bad argument");
    const int64_t skip = head_skip < n_data ? head_skip : n_data;
    if (h->filled + (n_data - skip) > h->n_bytes)
        return dn::fail(DN_E_INVALID, "dn_bam_sort_window_host: the blocks hold more bytes than dn_bam_sort_create was told");
    if (n_data > skip) memcpy(h->h_in.data() + h->filled, data + skip, (size_t) (n_data - skip));
    h->filled += n_data - skip;
    h->n_windows++;
    return DN_OK;
}

extern "C" int dn_bam_sort_finish(dn_bam_sort h, int64_t *n_records, int64_t *n_bytes, int64_t *n_fixups, double *frame_ms, double *sort_ms,
                                  double *gather_ms)
{
    dn::clear_error();
    if (!h || !n_records || !n_bytes) return dn::fail(DN_E_INVALID, "dn_bam_sort_finish: bad argument");
    if (h->failed || h->finished) return dn::fail(DN_E_STATE, "dn_bam_sort_finish: the sort is finished or has failed");
    if (h->filled != h->n_bytes) {
        h->failed = true;
        return dn::fail(DN_E_INVALID, "dn_bam_sort_finish: " + std::to_string(h->filled) + " bytes were handed over, dn_bam_sort_create was told " +
                                      std::to_string(h->n_bytes));
    }
    HostSort hs{h};
    DeviceSort ds{h};
    uint32_t top = 0;
    int64_t total = 0;
    const auto body = [&]() -> int {
        int rc = h->device < 0 ? run_sort(h, hs, top) : run_sort(h, ds, top);
        if (rc != DN_OK) return rc;
        if (h->device >= 0) top = ds.top();
        const int pos_bits = bits_of(top), ref_bits = bits_of((uint64_t) h->n_ref);
        rc = h->device < 0 ? hs.sort_and_gather(pos_bits, ref_bits, total) : ds.sort_and_gather(pos_bits, ref_bits, total);
        if (rc != DN_OK) { h->failed = true; return rc; }
        if (total != h->n_bytes) {
            h->failed = true;
            return dn::fail(DN_E_STATE, "dn_bam_sort_finish: the records hold " + std::to_string(total) + " of the stream's " + std::to_string(h->n_bytes) + " bytes");
        }
        return DN_OK;
    };
    int rc;
    if (h->device < 0) {
        rc = body();
    } else {
        DN_TRY(hipSetDevice(h->device));
        rc = dn::synced(h->st, body);
    }
    if (rc != DN_OK) return rc;
    h->finished = true;
    *n_records = h->n_records;
    *n_bytes = h->n_bytes;
    if (n_fixups) *n_fixups = h->n_fixups;
    if (frame_ms) *frame_ms = h->frame_ms;
    if (sort_ms) *sort_ms = ds.sort_ms;
    if (gather_ms) *gather_ms = ds.gather_ms;
    return DN_OK;
}

extern "C" int dn_bam_sort_ends(dn_bam_sort h, int64_t first, int64_t n, int64_t *ends)
{
    dn::clear_error();
    if (!h || first < 0 || n < 0 || (n > 0 && !ends)) return dn::fail(DN_E_INVALID, "dn_bam_sort_ends: bad argument");
    if (!h->finished) return dn::fail(DN_E_STATE, "dn_bam_sort_ends: dn_bam_sort_finish first");
    if (first > h->n_records || n > h->n_records - first) return dn::fail(DN_E_INVALID, "dn_bam_sort_ends: records outside the file");
    if (n == 0) return DN_OK;
    if (h->device < 0) {
        std::copy(h->h_dst.begin() + first + 1, h->h_dst.begin() + first + 1 + n, ends);
        return DN_OK;
    }
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(hipMemcpyAsync(ends, h->dst + (first + 1), sizeof(int64_t) * (size_t) n, hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    });
}

extern "C" int dn_bam_sort_read(dn_bam_sort h, int64_t off, int64_t n, uint8_t *dst)
{
    dn::clear_error();
    if (!h || off < 0 || n < 0 || (n > 0 && !dst)) return dn::fail(DN_E_INVALID, "dn_bam_sort_read: bad argument");
    if (!h->finished) return dn::fail(DN_E_STATE, "dn_bam_sort_read: dn_bam_sort_finish first");
    if (off > h->n_bytes || n > h->n_bytes - off) return dn::fail(DN_E_INVALID, "dn_bam_sort_read: bytes outside the stream");
    if (n == 0) return DN_OK;
    if (h->device < 0) {
        memcpy(dst, h->h_out.data() + off, (size_t) n);
        return DN_OK;
    }
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->st, [&]() -> int {
        DN_TRY(hipMemcpyAsync(dst, h->out + off, (size_t) n, hipMemcpyDeviceToHost, h->st));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    });
}

extern "C" int dn_bam_sort_deflate(dn_bam_sort h, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *out, int64_t out_cap,
                                   int64_t *out_off, double *deflate_ms)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bam_sort_deflate: bad argument");
    if (!h->finished || h->failed) return dn::fail(DN_E_STATE, "dn_bam_sort_deflate: the sort is not finished or has failed");
    const int rc = dn::deflate_validate("dn_bam_sort_deflate", h->n_bytes, n_blocks, beg, len, out, out_cap, out_off);
    if (rc != DN_OK) return rc;
    if (deflate_ms) *deflate_ms = 0.0;
    if (h->device < 0) return dn::deflate_host(h->h_out.data(), h->n_bytes, n_blocks, beg, len, out, out_off);
    DN_TRY(hipSetDevice(h->device));
    const int rc2 = dn::synced(h->st, [&]() -> int {
        if (!h->deflating) {
            // what only the sort needed goes: the deflate tables are smaller, so the device need stays below the sort's
            DN_TRY(hipStreamSynchronize(h->st));
            h->ingest = dn::InflateWindow();
            h->piece_off = dn::GrowBuffer<int64_t>(); h->off = dn::GrowBuffer<int64_t>();
            h->key = dn::GrowBuffer<uint64_t>(); h->key2 = dn::GrowBuffer<uint64_t>();
            h->ord = dn::GrowBuffer<uint32_t>(); h->ord2 = dn::GrowBuffer<uint32_t>(); h->len = dn::GrowBuffer<uint32_t>();
            h->deflating = true;
        }
        // the unsorted copy of the stream is dead since the gather: it holds the slots and the compacted blocks
        uint8_t *region = h->in.get();
        int64_t region_bytes = (h->n_bytes + kSlack) & ~(int64_t) 15;
        if (region_bytes < dn::kDeflateRegionPerBlock) {
            region_bytes = dn::kDeflateRegionPerBlock;
            if (!h->deflate_region) DN_TRY(h->deflate_region.alloc((size_t) region_bytes));
            region = h->deflate_region.get();
        }
        return dn::deflate_device(h->st, h->out.get(), n_blocks, beg, len, region, region_bytes, h->deflate, out, out_off, deflate_ms);
    });
    if (rc2 != DN_OK) h->failed = true;
    return rc2;
}

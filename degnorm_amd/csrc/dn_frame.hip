// dn_frame.hip -- where the records of an inflated BAM window start, found on the device.
//
// A record's start is known only from the record before it (block_size to block_size), so dn_bam_frame (dn_reads.hip) walks
// a window serially.  Here the window is cut into segments of S bytes and the chain is walked in all of them at once:
//
//   guess    one wavefront per segment tests 64 consecutive offsets per step against a plausibility rule (frame_plausible)
//            and takes the first that passes as the segment's entry; segment 0 enters at offset 0, which is true by definition
//   walk     one lane per segment follows block_size from the entry to the first offset at or beyond the segment's end,
//            or to the window's tail, and leaves a FrameSeg: records counted, exit offset, last pos, state.  A block_size
//            below 32 met here is a state, not an error: the entry may have been a wrong guess
//   stitch   the host reads the table of FrameSegs (32 bytes per segment, no window byte) and follows it from offset 0: the
//            true entry of a segment is the exit of the last segment the true chain passed through; a segment the chain
//            jumps over (a record longer than a segment) contributes nothing; where the true entry differs from the guess,
//            that segment alone is walked again from the true entry (a fix-up: one small launch) and the stitch goes on.
//            By induction from offset 0 the result is the serial chain, whatever the guesses were
//   emit     the counts of the segments on the chain are scanned, and one lane per segment walks its records again, writes
//            their offsets and applies dn_bam_frame's order check (refID == tid, pos not below the pos before)
//
// Worst case: every guess is wrong.  Then the stitch costs one small launch and one 32-byte copy per segment, the same
// order of time as the serial host walk it replaces.  There is no cap on fix-ups and no other path.
//
// Guess, walk and emit of one segment are __host__ __device__ functions; dn_bam_frame_segments_host runs them in plain
// loops under the same stitch, so the whole algorithm, fix-ups included, is testable without a device.  Every read is
// checked against n_bytes first: garbage yields a state, never an access outside the window.  The readers and the offsets
// of the fixed fields are those of dn_bam_record.hpp; the rules below are this unit's own.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_frame.hpp"
#include "dn_bam_record.hpp"

namespace {

using dn::le16;
using dn::le32;

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int64_t kGridCap = 1 << 20;

// The fixed fields of the record at o (o + 36 <= n_bytes is the caller's): of tid, and sized within block_size bs.  Beyond
// what a record must satisfy, the guess also wants what records of real files satisfy -- a read name of at least one
// character (l_read_name >= 2) and pos, next_refID, next_pos no less than -1 -- because the commonest false start, the last
// byte of a record that ends in a zero byte followed by the next record's first bytes, fails exactly these.  A true record
// that fails them costs a fix-up, never a wrong result.
DN_HD bool frame_fields_ok(const uint8_t *w, int64_t o, int32_t bs, int32_t tid)
{
    const uint8_t *p = w + o;
    if (tid >= 0 && (int32_t) le32(p + dn::kBamRef) != tid) return false;
    const int64_t l_name = p[dn::kBamLName], n_cig = le16(p + dn::kBamNCigar);
    const int32_t l_seq = (int32_t) le32(p + dn::kBamLSeq);
    if (l_name < 2 || l_seq < 0) return false;
    if ((int32_t) le32(p + dn::kBamPos) < -1 || (int32_t) le32(p + dn::kBamNextRef) < -1 || (int32_t) le32(p + dn::kBamNextPos) < -1) return false;
    return dn::kBamMinSize + l_name + 4 * n_cig + ((int64_t) l_seq + 1) / 2 + l_seq <= bs;
}

constexpr int kFrameLookAhead = 2;      // records behind a candidate whose fixed fields must look right too

// Could a record start at p?  It fits the window, its fields pass frame_fields_ok, its read name ends with NUL, and
// whatever of the fixed parts of the kFrameLookAhead records behind it is inside the window passes frame_fields_ok too.
DN_HD bool frame_plausible(const uint8_t *w, int64_t n_bytes, int64_t p, int32_t tid)
{
    if (p < 0 || p + dn::kBamName > n_bytes) return false;
    int32_t bs = (int32_t) le32(w + p);
    if (bs < dn::kBamMinSize || p + 4 + (int64_t) bs > n_bytes) return false;
    if (!frame_fields_ok(w, p, bs, tid)) return false;
    if (w[p + dn::kBamName + w[p + dn::kBamLName] - 1] != 0) return false;    // inside the record: 32 + l_read_name <= bs
    int64_t q = p;
    for (int k = 0; k < kFrameLookAhead; k++) {
        q += 4 + (int64_t) bs;
        if (q + dn::kBamName > n_bytes) return true;
        bs = (int32_t) le32(w + q);
        if (bs < dn::kBamMinSize || !frame_fields_ok(w, q, bs, tid)) return false;
    }
    return true;
}

// Follow the chain from `entry` to the first offset >= limit or to the window's tail.  The tail rule is dn_bam_frame's: a
// block_size that is visible and below 32 is kFrameBad even when its record is cut by the window end.
DN_HD dn::FrameSeg frame_walk(const uint8_t *w, int64_t n_bytes, int64_t entry, int64_t limit)
{
    dn::FrameSeg G{entry, entry, 0, 0, dn::kFrameOk, 0};
    int64_t o = entry;
    while (o < limit) {
        if (o + 4 > n_bytes) { G.state = dn::kFrameTail; break; }
        const int32_t bs = (int32_t) le32(w + o);
        if (bs < dn::kBamMinSize) { G.state = dn::kFrameBad; G.bad_bs = bs; break; }
        if (o + 4 + (int64_t) bs > n_bytes) { G.state = dn::kFrameTail; break; }
        G.last_pos = (int32_t) le32(w + o + dn::kBamPos);
        G.count++;
        o += 4 + (int64_t) bs;
    }
    G.exit = o;
    return G;
}

// Walk G's records again from its entry: their offsets to rec_off[base ..], and the index of the first one that fails
// dn_bam_frame's order check (-1: none; prev is the pos of the record before G's first).  The bounds were established by
// the walk that counted the records; they are checked again so that a table that does not belong to w cannot lead outside.
DN_HD int64_t frame_emit(const uint8_t *w, int64_t n_bytes, const dn::FrameSeg &G, int32_t prev, int32_t tid, int64_t base,
                         int64_t *rec_off)
{
    int64_t o = G.entry, bad = -1;
    for (int32_t i = 0; i < G.count; i++) {
        if (o < 0 || o + dn::kBamPosEnd > n_bytes) break;
        const int32_t bs = (int32_t) le32(w + o);
        if (bs < dn::kBamMinSize) break;
        rec_off[base + i] = o;
        if (tid >= 0) {
            const int32_t ref = (int32_t) le32(w + o + dn::kBamRef), pos = (int32_t) le32(w + o + dn::kBamPos);
            if ((ref != tid || pos < prev) && bad < 0) bad = base + i;
            prev = pos;
        }
        o += 4 + (int64_t) bs;
    }
    return bad;
}

DN_HD int64_t segment_end(int64_t s, int64_t S, int64_t n_bytes) { return (s + 1) * S < n_bytes ? (s + 1) * S : n_bytes; }

// the guess of segment s > 0 on the host: the first plausible offset, -1 without one
int64_t frame_guess_host(const uint8_t *w, int64_t n_bytes, int64_t s, int64_t S, int32_t tid)
{
    for (int64_t p = s * S; p < segment_end(s, S, n_bytes); p++)
        if (frame_plausible(w, n_bytes, p, tid)) return p;
    return -1;
}

// one wavefront per segment: 64 offsets per step, the first set bit of the ballot
__global__ __launch_bounds__(kNT) void k_frame_guess(const uint8_t *__restrict__ w, int64_t n_bytes, int32_t tid, int64_t S, int64_t n_seg,
                                                     dn::FrameSeg *__restrict__ seg)
{
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t s = (int64_t) blockIdx.x * (kNT / kWave) + threadIdx.x / kWave; s < n_seg; s += (int64_t) gridDim.x * (kNT / kWave)) {
        int64_t entry = s == 0 ? 0 : -1;
        const int64_t end = segment_end(s, S, n_bytes);
        for (int64_t p0 = s * S; s > 0 && p0 < end; p0 += kWave) {           // p0, end: the same in every lane of the wave
            const int64_t p = p0 + lane;
            const unsigned long long m = __ballot(p < end && frame_plausible(w, n_bytes, p, tid));
            if (m) { entry = p0 + __ffsll(m) - 1; break; }
        }
        if (lane == 0) seg[s].entry = entry;
    }
}

// one lane per segment of [s0, s0 + n): walk from seg[s].entry, or from `entry` when it is >= 0 (a fix-up: n == 1)
__global__ __launch_bounds__(kNT) void k_frame_walk(const uint8_t *__restrict__ w, int64_t n_bytes, int64_t S, int64_t s0, int64_t n,
                                                    int64_t entry, dn::FrameSeg *__restrict__ seg)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) {
        const int64_t s = s0 + i, e = entry >= 0 ? entry : seg[s].entry;
        seg[s] = e >= 0 ? frame_walk(w, n_bytes, e, (s + 1) * S) : dn::FrameSeg{-1, -1, 0, 0, dn::kFrameOk, 0};
    }
}

__global__ __launch_bounds__(kNT) void k_frame_counts(int64_t n_seg, const dn::FrameSeg *__restrict__ seg, const dn::FramePlan *__restrict__ plan,
                                                      int32_t *__restrict__ cnt)
{
    for (int64_t s = (int64_t) blockIdx.x * kNT + threadIdx.x; s < n_seg; s += (int64_t) gridDim.x * kNT)
        cnt[s] = plan[s].active ? seg[s].count : 0;
}

__global__ __launch_bounds__(kNT) void k_frame_emit(const uint8_t *__restrict__ w, int64_t n_bytes, int32_t tid, int64_t n_seg,
                                                    const dn::FrameSeg *__restrict__ seg, const dn::FramePlan *__restrict__ plan,
                                                    const int32_t *__restrict__ base, int64_t *__restrict__ rec_off,
                                                    unsigned long long *__restrict__ err)
{
    for (int64_t s = (int64_t) blockIdx.x * kNT + threadIdx.x; s < n_seg; s += (int64_t) gridDim.x * kNT) {
        if (!plan[s].active) continue;
        const int64_t bad = frame_emit(w, n_bytes, seg[s], plan[s].prev_pos, tid, base[s], rec_off);
        if (bad >= 0) atomicMin(err, (unsigned long long) bad);
    }
}

// the segments walked in a plain loop on the host
struct HostFrame {
    const uint8_t *w;
    int64_t n_bytes, S, n_seg;
    int32_t tid;
    std::vector<dn::FrameSeg> T;
    std::vector<dn::FramePlan> plan;
    std::vector<int64_t> off;

    int table()
    {
        for (int64_t s = 0; s < n_seg; s++) {
            const int64_t e = s == 0 ? 0 : frame_guess_host(w, n_bytes, s, S, tid);
            T[(size_t) s] = e >= 0 ? frame_walk(w, n_bytes, e, (s + 1) * S) : dn::FrameSeg{-1, -1, 0, 0, dn::kFrameOk, 0};
        }
        return DN_OK;
    }
    int fixup(int64_t s, int64_t entry, dn::FrameSeg &G)
    {
        G = frame_walk(w, n_bytes, entry, (s + 1) * S);
        return DN_OK;
    }
    int emit(int64_t n_rec, int64_t &first_bad)
    {
        off.resize((size_t) n_rec + 1);
        int64_t base = 0;
        for (int64_t s = 0; s < n_seg; s++) {
            if (!plan[(size_t) s].active) continue;
            const int64_t bad = frame_emit(w, n_bytes, T[(size_t) s], plan[(size_t) s].prev_pos, tid, base, off.data());
            if (bad >= 0 && (first_bad < 0 || bad < first_bad)) first_bad = bad;
            base += T[(size_t) s].count;
        }
        return DN_OK;
    }
    int record(int64_t i, int32_t &ref, int32_t &pos)
    {
        ref = (int32_t) le32(w + off[(size_t) i] + dn::kBamRef);
        pos = (int32_t) le32(w + off[(size_t) i] + dn::kBamPos);
        return DN_OK;
    }
};

// the same on the device; every call queues its work on st and waits where the host reads a result.  What the queued
// copies write lives in this object: frame_window declares it outside the body it hands to dn::synced
struct DeviceFrame {
    hipStream_t st;
    dn::FrameWork &W;
    const uint8_t *w;
    int64_t n_bytes, S, n_seg;
    int32_t tid;
    dn::GrowBuffer<int64_t> &rec_off;
    std::vector<dn::FrameSeg> T;
    std::vector<dn::FramePlan> plan;
    unsigned long long h_err = ~0ull;
    int64_t h_off = 0;
    uint8_t h_rec[dn::kBamPosEnd] = {0};

    int table()
    {
        DN_TRY(W.seg.reserve(n_seg, 0, st));
        hipLaunchKernelGGL(k_frame_guess, dim3(dn::grid_for(n_seg, kNT / kWave, kGridCap)), dim3(kNT), 0, st, w, n_bytes, tid, S, n_seg, W.seg.get());
        DN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_frame_walk, dim3(dn::grid_for(n_seg, kNT, kGridCap)), dim3(kNT), 0, st, w, n_bytes, S, (int64_t) 0, n_seg, (int64_t) -1, W.seg.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(T.data(), W.seg, sizeof(dn::FrameSeg) * (size_t) n_seg, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        return DN_OK;
    }
    int fixup(int64_t s, int64_t entry, dn::FrameSeg &G)
    {
        hipLaunchKernelGGL(k_frame_walk, dim3(1), dim3(kNT), 0, st, w, n_bytes, S, s, (int64_t) 1, entry, W.seg.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&G, W.seg + s, sizeof(dn::FrameSeg), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        return DN_OK;
    }
    int emit(int64_t n_rec, int64_t &first_bad)
    {
        DN_TRY(rec_off.reserve(n_rec + 1, 0, st));
        DN_TRY(W.plan.reserve(n_seg, 0, st)); DN_TRY(W.cnt.reserve(n_seg, 0, st)); DN_TRY(W.base.reserve(n_seg, 0, st));
        if (!W.err) DN_TRY(dn::alloc_padded(W.err, 1));
        DN_TRY(hipMemcpyAsync(W.plan, plan.data(), sizeof(dn::FramePlan) * (size_t) n_seg, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemsetAsync(W.err, 0xff, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_frame_counts, dim3(dn::grid_for(n_seg, kNT, kGridCap)), dim3(kNT), 0, st, n_seg, W.seg.get(), W.plan.get(), W.cnt.get());
        DN_TRY(hipGetLastError());
        DN_TRY(W.scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, W.cnt.get(), W.base.get(), (int) n_seg, st);
        }));
        hipLaunchKernelGGL(k_frame_emit, dim3(dn::grid_for(n_seg, kNT, kGridCap)), dim3(kNT), 0, st, w, n_bytes, tid, n_seg, W.seg.get(), W.plan.get(),
                           W.base.get(), rec_off.get(), W.err.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&h_err, W.err, sizeof(h_err), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (h_err != ~0ull) first_bad = (int64_t) h_err;
        return DN_OK;
    }
    int record(int64_t i, int32_t &ref, int32_t &pos)
    {
        DN_TRY(hipMemcpyAsync(&h_off, rec_off + i, sizeof(h_off), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (h_off < 0 || h_off + dn::kBamPosEnd > n_bytes) return dn::fail(DN_E_STATE, "frame_window: record offset outside the window");
        DN_TRY(hipMemcpyAsync(h_rec, w + h_off, sizeof(h_rec), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        ref = (int32_t) le32(h_rec + dn::kBamRef);
        pos = (int32_t) le32(h_rec + dn::kBamPos);
        return DN_OK;
    }
};

// Table, stitch, emit and dn_bam_frame's verdict, on either backend.  cap < 0: no limit on the number of records.
template <class B> int frame_run(B &be, int32_t *last_pos, int64_t cap, dn::FrameResult &R)
{
    const int64_t n_seg = be.n_seg, S = be.S;
    std::vector<dn::FrameSeg> &T = be.T;
    std::vector<dn::FramePlan> &plan = be.plan;
    T.assign((size_t) n_seg, dn::FrameSeg{-1, -1, 0, 0, dn::kFrameOk, 0});
    plan.assign((size_t) n_seg, dn::FramePlan{0, 0});
    const int32_t first_prev = last_pos ? *last_pos : INT32_MIN;
    int32_t prev = first_prev, state = dn::kFrameOk, bad_bs = 0;
    int64_t cur = 0, n_rec = 0, fixups = 0;
    int rc = n_seg > 0 ? be.table() : DN_OK;
    if (rc != DN_OK) return rc;
    // cur is a true record start inside segment s, by induction: every exit of a walk from a true start is one, and an
    // exit with state ok lies at or beyond its segment's end, so s grows and segments the chain jumps over stay inactive
    for (int64_t s = 0; s < n_seg; s = cur / S) {
        dn::FrameSeg &G = T[(size_t) s];
        if (G.entry != cur) {
            if ((rc = be.fixup(s, cur, G)) != DN_OK) return rc;
            fixups++;
        }
        plan[(size_t) s] = dn::FramePlan{1, prev};
        n_rec += G.count;
        if (G.count > 0) prev = G.last_pos;
        cur = G.exit;
        state = G.state;
        bad_bs = G.bad_bs;
        if (state != dn::kFrameOk) break;
    }
    R.n_segments = n_seg;
    R.n_fixups = fixups;
    int64_t first_bad = -1;
    if (n_rec > 0 && (rc = be.emit(n_rec, first_bad)) != DN_OK) return rc;
    // in file order, as the serial walk meets them: a record out of order, the record beyond cap, the malformed record
    if (first_bad >= 0 && (cap < 0 || first_bad < cap)) {
        int32_t ref = 0, pos = 0, before = first_prev;
        if (first_bad > 0 && (rc = be.record(first_bad - 1, ref, before)) != DN_OK) return rc;
        if ((rc = be.record(first_bad, ref, pos)) != DN_OK) return rc;
        return dn::fail(DN_E_INVALID, "BAM file is not sorted by coordinate, or its index is stale: a record of refID " + std::to_string(ref) +
                                      " at position " + std::to_string(pos) + " follows position " + std::to_string(before) +
                                      " inside the index range of refID " + std::to_string(be.tid));
    }
    if (cap >= 0 && n_rec > cap) return dn::fail(DN_E_INVALID, "dn_bam_frame: more records than cap");
    if (state == dn::kFrameBad) {
        R.n_rec = n_rec;
        R.consumed = cur;
        R.bad = true;
        R.bad_bs = bad_bs;
        return dn::fail(DN_E_INVALID, "malformed BAM record at byte " + std::to_string(cur) + " of the window (block_size " + std::to_string(bad_bs) + ")");
    }
    if (be.tid >= 0 && n_rec > 0) *last_pos = prev;
    R.n_rec = n_rec;
    R.consumed = cur;
    return DN_OK;
}

int frame_args(const char *who, const uint8_t *buf, int64_t n_bytes, int32_t tid, const int32_t *last_pos, int64_t &segment_bytes,
               const int64_t *rec_off, int64_t cap, const int64_t *n_rec, const int64_t *consumed)
{
    if (n_bytes < 0 || (n_bytes > 0 && !buf) || cap < 0 || (cap > 0 && !rec_off) || !n_rec || !consumed || (tid >= 0 && !last_pos))
        return dn::fail(DN_E_INVALID, std::string(who) + ": bad argument");
    if (segment_bytes == 0) segment_bytes = dn::kFrameSegmentDefault;
    if (segment_bytes < dn::kFrameSegmentMin) return dn::fail(DN_E_INVALID, std::string(who) + ": segment_bytes below 64");
    return DN_OK;
}

}  // namespace

int dn::frame_window(hipStream_t st, FrameWork &W, const uint8_t *d_win, int64_t n_bytes, int32_t tid, int32_t *last_pos,
                     int64_t segment_bytes, int64_t cap, GrowBuffer<int64_t> &rec_off, FrameResult &R)
{
    const int64_t S = segment_bytes == 0 ? kFrameSegmentDefault : segment_bytes;
    if (n_bytes < 0 || n_bytes > INT32_MAX || S < kFrameSegmentMin || (tid >= 0 && !last_pos))
        return dn::fail(DN_E_INVALID, "frame_window: bad argument");
    DeviceFrame be{st, W, d_win, n_bytes, S, (n_bytes + S - 1) / S, tid, rec_off, {}, {}};
    return dn::synced(st, [&]() -> int {
        if (!W.ev0) { DN_TRY(W.ev0.create(hipEventCreate)); DN_TRY(W.ev1.create(hipEventCreate)); }
        DN_TRY(hipEventRecord(W.ev0, st));
        const int rc = frame_run(be, last_pos, cap, R);
        DN_TRY(hipEventRecord(W.ev1, st));
        DN_TRY(hipStreamSynchronize(st));
        DN_TRY(hipEventElapsedTime(&R.device_ms, W.ev0, W.ev1));
        return rc;
    });
}

extern "C" int64_t dn_bam_frame_segment_default(void) { return dn::kFrameSegmentDefault; }

extern "C" int dn_bam_frame_segments_host(const uint8_t *buf, int64_t n_bytes, int32_t tid, int32_t *last_pos, int64_t segment_bytes,
                                          int64_t *rec_off, int64_t cap, int64_t *n_rec, int64_t *consumed, int64_t *n_fixups)
{
    dn::clear_error();
    int rc = frame_args("dn_bam_frame_segments_host", buf, n_bytes, tid, last_pos, segment_bytes, rec_off, cap, n_rec, consumed);
    if (rc != DN_OK) return rc;
    HostFrame be{buf, n_bytes, segment_bytes, (n_bytes + segment_bytes - 1) / segment_bytes, tid, {}, {}, {}};
    dn::FrameResult R;
    rc = frame_run(be, last_pos, cap, R);
    if (n_fixups) *n_fixups = R.n_fixups;
    if (rc != DN_OK) return rc;
    for (int64_t i = 0; i < R.n_rec; i++) rec_off[i] = be.off[(size_t) i];
    *n_rec = R.n_rec;
    *consumed = R.consumed;
    return DN_OK;
}

extern "C" int dn_bam_frame_device(int device, const uint8_t *buf, int64_t n_bytes, int32_t tid, int32_t *last_pos, int64_t segment_bytes,
                                   int64_t *rec_off, int64_t cap, int64_t *n_rec, int64_t *consumed, int64_t *n_fixups, double *device_ms)
{
    dn::clear_error();
    int rc = frame_args("dn_bam_frame_device", buf, n_bytes, tid, last_pos, segment_bytes, rec_off, cap, n_rec, consumed);
    if (rc != DN_OK) return rc;
    if (n_bytes > INT32_MAX) return dn::fail(DN_E_INVALID, "dn_bam_frame_device: window beyond 2^31 - 1 bytes");
    dn::Stream st;
    dn::FrameWork W;
    dn::DeviceBuffer<uint8_t> d_win;
    dn::GrowBuffer<int64_t> d_off;
    dn::FrameResult R;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(dn::alloc_padded(d_win, (size_t) n_bytes));
        if (n_bytes > 0) DN_TRY(hipMemcpyAsync(d_win, buf, (size_t) n_bytes, hipMemcpyHostToDevice, st));
        const int frc = dn::frame_window(st, W, d_win, n_bytes, tid, last_pos, segment_bytes, cap, d_off, R);
        if (n_fixups) *n_fixups = R.n_fixups;
        if (device_ms) *device_ms = R.device_ms;
        if (frc != DN_OK) return frc;
        if (R.n_rec > 0) DN_TRY(hipMemcpyAsync(rec_off, d_off, sizeof(int64_t) * (size_t) R.n_rec, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        *n_rec = R.n_rec;
        *consumed = R.consumed;
        return DN_OK;
    });
}

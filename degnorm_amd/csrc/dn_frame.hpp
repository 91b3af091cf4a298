// dn_frame.hpp -- what the reads unit (dn_reads.hip) needs of the record-framing unit (dn_frame.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dn_host.hpp"

namespace dn {

constexpr int64_t kFrameSegmentMin = 64;
constexpr int64_t kFrameSegmentDefault = 16384;     // bytes of a window one segment covers when the caller passes 0

enum { kFrameOk = 0, kFrameTail = 1, kFrameBad = 2 };

// What the walk of one segment found.  entry: where it started (-1: the segment has no plausible offset and was not
// walked); exit: where it stopped -- the first record start at or beyond the segment's end (kFrameOk), the record cut by
// the window end (kFrameTail) or the record whose block_size, bad_bs, is below 32 (kFrameBad); count records lie in
// [entry, exit) and last_pos is the pos of the last of them.
struct FrameSeg {
    int64_t entry, exit;
    int32_t count, last_pos, state, bad_bs;
};

// What the host's stitch tells the emit pass about a segment: whether the true chain enters it (at FrameSeg::entry), and
// the pos of the record before its first one.
struct FramePlan {
    int32_t active, prev_pos;
};

// device memory and events of frame_window; kept by the caller from window to window
struct FrameWork {
    GrowBuffer<FrameSeg> seg;
    GrowBuffer<FramePlan> plan;
    GrowBuffer<int32_t> cnt, base;
    DeviceBuffer<unsigned long long> err;
    Scratch scratch;
    Event ev0, ev1;
};

struct FrameResult {
    int64_t n_rec = 0, consumed = 0, n_segments = 0, n_fixups = 0;
    float device_ms = 0.f;              // first framing kernel to the last, the host's stitch between them included
    // when the walk stopped at a record whose block_size is below 32 (the call then fails): n_rec records lie before it, it
    // starts at `consumed`, and bad_bs is its block_size
    bool bad = false;
    int32_t bad_bs = 0;
};

// Frame the n_bytes of the device window d_win on stream st: what dn_bam_frame does on the host, with the same results and
// the same errors (a DN_* code; text in the library's error channel), more than cap records among them (cap < 0: no limit).
// rec_off is grown to R.n_rec + 1 entries and receives the record offsets; *last_pos is read and, on success with tid >= 0,
// updated.  segment_bytes 0: kFrameSegmentDefault.  The stream is idle when the call returns.
int frame_window(hipStream_t st, FrameWork &W, const uint8_t *d_win, int64_t n_bytes, int32_t tid, int32_t *last_pos,
                 int64_t segment_bytes, int64_t cap, GrowBuffer<int64_t> &rec_off, FrameResult &R);

}  // namespace dn

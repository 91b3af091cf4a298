// dn_inflate.hpp -- what the units that take BGZF blocks (dn_reads.hip, dn_bai.hip, dn_sort.hip) need of the inflate unit
// (dn_inflate.hip): the launch, and the window ingest they share (InflateWindow, DeviceCarry).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dn_host.hpp"

namespace dn {

// One BGZF block of a launch.  Its raw-deflate payload is comp[pay_off .. pay_off + pay_len) and must inflate to exactly
// isize bytes; of those, bytes [skip, skip + keep) are written to out[dst_off ..).  With check != 0 the CRC32 of all isize
// bytes must be crc (the block's trailer), else the block's status is DN_INFLATE_E_CRC.
struct InflateBlock {
    int64_t pay_off, dst_off;
    int32_t pay_len, isize, skip, keep;
    uint32_t crc;
    int32_t check;
};

// bytes a device copy of n_comp compressed bytes must be allocated with (the kernel reads it in whole 16-byte pieces)
inline int64_t inflate_comp_cap(int64_t n_comp) { return ((n_comp + 15) & ~(int64_t) 15) + 16; }

// one wave per block on stream st; d_status[b] = 0 or DN_INFLATE_E_*.  The arrays were validated by the caller.
hipError_t inflate_launch(hipStream_t st, const uint8_t *d_comp, int64_t comp_cap, const InflateBlock *d_blk, int64_t n_blocks,
                          uint8_t *d_out, int32_t *d_status);

inline bool payload_inside(int64_t pay_off, int32_t pay_len, int64_t n_comp)
{
    return pay_off >= 0 && pay_len >= 0 && pay_off <= n_comp && pay_len <= n_comp - pay_off;
}

// The bytes [skip, skip + keep) that a window holds of block b of its n_blocks, which inflates to isize >= 0 bytes: the
// window starts head_skip bytes into its first block and ends tail_keep bytes into its last one (-1: at its end).  The last
// block is cut first, then the first one.
inline void window_trim(int64_t b, int64_t n_blocks, int32_t isize, int32_t head_skip, int32_t tail_keep, int32_t &skip, int32_t &keep)
{
    int32_t hi = isize;
    if (b == n_blocks - 1 && tail_keep >= 0 && tail_keep < hi) hi = tail_keep;
    skip = b == 0 ? (head_skip < hi ? head_skip : hi) : 0;
    keep = hi - skip;
}

// a window is indexed with 32 bits: what the entry point `who` says of one that is larger
inline int window_size_error(const char *who) { return fail(DN_E_INVALID, std::string(who) + ": window beyond 2^31 - 1 bytes"); }

// The window ingest: a batch of BGZF blocks, as they lie in the file, inflated to a place on the device, checked against
// their trailer CRC32s when these were announced.  One per handle; an entry point that takes a window calls take() first,
// then its own checks, plan() and, inside its dn::synced body, run() -- or queue(), copies of its own, and wait().
struct InflateWindow {
    GrowBuffer<uint8_t> comp;
    GrowBuffer<InflateBlock> d_blk;
    GrowBuffer<int32_t> d_status;
    Event ev0, ev1;                           // around the kernel; created on first use
    std::vector<uint32_t> announced, crc;     // by arm() for the next call; of the current call
    bool armed = false, checking = false;
    std::vector<InflateBlock> blk;            // of the current call

    // the body of an *_expect_crc entry point `who`: the next call checks its blocks against these CRC32s, one per block
    int arm(const char *who, const uint32_t *crc32, int64_t n_blocks);

    // The announced CRC32s become this call's and the arming is spent, whatever the call then returns: so before any check.
    void take()
    {
        checking = armed;
        crc.swap(announced);
        announced.clear();
        armed = false;
    }

    // The descriptors of the call `who` (armed by `armed_by`): block b writes its trimmed bytes (window_trim) behind those of
    // the blocks before it, the first one at out[base ..); total = where the window ends.  DN_E_INVALID for a CRC count that
    // is not n_blocks, a negative size or a payload outside comp.
    int plan(const char *who, const char *armed_by, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
             const int32_t *isize, int32_t head_skip, int32_t tail_keep, int64_t base, int64_t &total);

    // queue: upload the planned blocks, inflate them into d_out on st and copy the statuses back.  wait: for st; *ms (nullable)
    // = the kernel's time, ok = every status is 0 (a block that failed left its bytes unspecified: the caller reports it).
    int queue(hipStream_t st, const uint8_t *comp_bytes, int64_t n_comp, uint8_t *d_out, int32_t *status);
    int wait(hipStream_t st, const int32_t *status, double *ms, bool &ok);
    int run(hipStream_t st, const uint8_t *comp_bytes, int64_t n_comp, uint8_t *d_out, int32_t *status, double *ms, bool &ok)
    {
        const int rc = queue(st, comp_bytes, n_comp, d_out, status);
        return rc != DN_OK ? rc : wait(st, status, ms, ok);
    }
};

// The record cut by a window's end, kept on the device while the window buffer is reused.
struct DeviceCarry {
    GrowBuffer<uint8_t> buf;
    int64_t n = 0;

    // the carried bytes -> the front of win (which has room for them)
    hipError_t put(hipStream_t st, uint8_t *win) const
    {
        return n > 0 ? hipMemcpyAsync(win, buf, (size_t) n, hipMemcpyDeviceToDevice, st) : hipSuccess;
    }
    // win[consumed .. total) is the next carry
    hipError_t keep(hipStream_t st, const uint8_t *win, int64_t consumed, int64_t total)
    {
        const int64_t left = total - consumed;
        hipError_t e = buf.reserve(left, 0, st);
        if (e == hipSuccess && left > 0) e = hipMemcpyAsync(buf, win + consumed, (size_t) left, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) n = left;
        return e;
    }
};

}  // namespace dn

// dn_inflate.hip -- raw DEFLATE (RFC 1951) decoder for BGZF blocks, one block per wavefront.
//
// A BGZF block is an independent raw-deflate stream of at most 64 KiB that names its own inflated size (ISIZE), so the
// blocks of a window inflate side by side.  The decoder (dn_inflate_core.hpp, shared with the gzip unit dn_gz.hip; a block is
// the span from bit 0 with no history: inflate_block below) is written once, as __host__ __device__ code against a memory
// policy M that says how input words, output bytes and the window of history are reached:
//
//   HostMem   plain arrays: the payload is read with bounds-checked loads, the output is written in place (and into a ring
//             of history, which a gzip segment preloads).  This is what
//             dn_bgzf_inflate_host runs, block after block, without a device: the build that is debugged and fuzzed.
//   WaveMem   one 64-lane workgroup (one wave) per block.  All 64 lanes run the bit reader and the symbol loop on the same
//             state (SIMT executes them at the price of one), so every branch is wave-uniform and nothing has to be
//             handed from a "decoding lane" to the others: a literal is stored by lane 0, a match is copied by all lanes,
//             and window refills and flushes are ordinary calls.  In LDS: the last 32 KiB of output as a ring (DEFLATE
//             reaches back at most 32768 bytes), a 2 KiB window of the payload, and the Huffman tables (38.9 KiB in
//             all: four workgroups per CU).  LDS operations of one wave execute in order, so a back-reference reads
//             what earlier instructions of the wave stored; wavefront-scope fences keep the compiler from reordering
//             them.  The ring is flushed to global memory with 16-byte stores before unflushed bytes would be
//             overwritten, and at the end.
//
// CRC32: with InflateBlock::check the policy keeps a running CRC register over every inflated byte (crc_slice, crc_join below).
// WaveMem does it in flush(), on the bytes the ring is about to release: every lane takes one contiguous slice from register
// 0, shifts it by the bytes behind it, and an xor across the wave joins the slices to the register carried from the flush
// before.  Bit by bit, without a table: no LDS beyond the 38.9 KiB above; measured, the pass adds 1.7-1.9 % to the kernel
// (about 5 cycles per byte against the 250 of the symbol loop; DESIGN.md, "BGZF inflate").  HostMem runs the same routines
// over its output array, lane after lane.
//
// Tables: a first-level lookup of 10 bits (literal/length) and 9 bits (distance) indexed by the next input bits, entry =
// symbol << 4 | code length, 0 = not in the table; longer codes (and codes that do not exist) take the canonical walk over
// count[len] / sorted symbols.  Input is untrusted: DESIGN.md ("BGZF inflate") has the bounds argument.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_inflate.hpp"

#define DN_HD __host__ __device__ __forceinline__
#include "dn_inflate_core.hpp"

namespace {

// Inflate one payload of n_in bytes into exactly isize bytes: the span from bit 0 with no history that stops at its final
// block (dn_inflate_core.hpp).  0 or DN_INFLATE_E_*.  With m.check the block must also have the CRC32 `crc` (m.crc starts at
// 0xffffffff); a decode error wins over DN_INFLATE_E_CRC.
template <class M> DN_HD int inflate_block(M &m, const Tables &t, int32_t n_in, int32_t isize, uint32_t crc)
{
    Stop stop{Stop::kFinal, 0, 0, nullptr, 0};
    stop.whole = true;
    Segment o;
    inflate_span(m, t, n_in, 0, stop, 0, isize, o);
    if (o.status) return o.status;
    if (o.out_len != isize) return DN_INFLATE_E_SIZE;
    if (((o.exit + 7) >> 3) != n_in) return DN_INFLATE_E_TRAILING;
    if (m.check && (m.crc ^ 0xffffffffu) != crc) return DN_INFLATE_E_CRC;
    return 0;
}

using BlockHost = HostMem<kBytes, int32_t>;      // a BGZF block is counted in 32 bits
using BlockWave = WaveMem<kBytes, int32_t>;

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *__restrict__ comp, int64_t comp_cap,
                                                     const dn::InflateBlock *__restrict__ blk, int64_t n_blocks,
                                                     uint8_t *__restrict__ out, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[kRing];
    __shared__ __attribute__((aligned(16))) uint32_t s_win[kWin / 4];
    __shared__ uint16_t s_lit[1 << kLitBits], s_dist[1 << kDistBits], s_sym_l[288], s_sym_d[32], s_cnt_l[16], s_cnt_d[16], s_offs[16];
    __shared__ uint8_t s_lens[320];
    const int64_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const dn::InflateBlock B = blk[b];
    Tables t{s_lit, s_dist, s_sym_l, s_sym_d, s_cnt_l, s_cnt_d, s_offs, s_lens};
    BlockWave m;
    m.tail = nullptr;
    m.ring = s_ring;
    m.win = s_win;
    m.comp = comp;
    m.comp_cap = comp_cap;
    m.abs0 = B.pay_off;
    m.wbase = -4 * (int64_t) kWin;
    m.dst = out + B.dst_off;
    m.skip = B.skip;
    m.keep = B.keep;
    m.flushed = 0;
    m.lane = (int) threadIdx.x;
    m.check = B.check != 0;
    m.crc = 0xffffffffu;
    const int rc = inflate_block(m, t, B.pay_len, B.isize, B.crc);
    if (threadIdx.x == 0) status[b] = rc;
}

int bad(const std::string &msg) { return dn::fail(DN_E_INVALID, msg); }

// the checks of the entry points; fills blk (skip 0, output at out_off[b]; out == nullptr, where the entry point allows it:
// nothing kept).  crc32 (nullable): the CRC32 every block must have.
int validate(const char *who, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
             const int64_t *out_off, const uint8_t *out, bool out_optional, const int32_t *status, const uint32_t *crc32,
             std::vector<dn::InflateBlock> &blk)
{
    const std::string w(who);
    if (n_comp < 0 || n_blocks < 0 || (n_comp > 0 && !comp) || !out_off || (n_blocks > 0 && (!pay_off || !pay_len || !status)))
        return bad(w + ": bad argument");
    if (out_off[0] != 0) return bad(w + ": out_off[0] is not 0");
    blk.resize((size_t) n_blocks);
    for (int64_t b = 0; b < n_blocks; b++) {
        const int64_t isize = out_off[b + 1] - out_off[b];
        if (!dn::payload_inside(pay_off[b], pay_len[b], n_comp)) return bad(w + ": payload of block " + std::to_string(b) + " outside comp");
        if (isize < 0 || isize > 65536) return bad(w + ": block " + std::to_string(b) + " has an inflated size outside 0 .. 65536");
        blk[(size_t) b] = dn::InflateBlock{pay_off[b], out ? out_off[b] : 0, pay_len[b], (int32_t) isize, 0, out ? (int32_t) isize : 0,
                                           crc32 ? crc32[b] : 0u, crc32 ? 1 : 0};
    }
    if (out_off[n_blocks] > 0 && !out && !out_optional) return bad(w + ": bad argument");
    return DN_OK;
}

int inflate_host(const char *who, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                 const int64_t *out_off, uint8_t *out, bool out_optional, int32_t *status, const uint32_t *crc32)
{
    dn::clear_error();
    std::vector<dn::InflateBlock> blk;
    const int rc = validate(who, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, out_optional, status, crc32, blk);
    if (rc != DN_OK) return rc;
    uint16_t lit[1 << kLitBits], dist[1 << kDistBits], sym_l[288], sym_d[32], cnt_l[16], cnt_d[16], offs[16];
    uint8_t lens[320];
    const Tables t{lit, dist, sym_l, sym_d, cnt_l, cnt_d, offs, lens};
    std::vector<uint8_t> dropped(out ? 0 : 65536), ring(kRing);
    for (const dn::InflateBlock &B : blk) {
        BlockHost m{comp + B.pay_off, ring.data(), out ? out + B.dst_off : dropped.data(), nullptr, B.check != 0};
        m.crc = 0xffffffffu;
        status[&B - blk.data()] = inflate_block(m, t, B.pay_len, B.isize, B.crc);
    }
    return DN_OK;
}

int inflate_device(const char *who, int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                   const int32_t *pay_len, const int64_t *out_off, uint8_t *out, bool out_optional, int32_t *status, double *copy_ms,
                   double *device_ms, const uint32_t *crc32)
{
    dn::clear_error();
    std::vector<dn::InflateBlock> blk;
    const int rc = validate(who, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, out_optional, status, crc32, blk);
    if (rc != DN_OK) return rc;
    if (copy_ms) *copy_ms = 0.0;
    if (device_ms) *device_ms = 0.0;
    if (n_blocks == 0) return DN_OK;
    if (n_blocks > INT32_MAX) return bad(std::string(who) + ": too many blocks");
    const int64_t n_out = out ? out_off[n_blocks] : 0, cap = dn::inflate_comp_cap(n_comp);
    dn::Stream st;
    dn::Event e0, e1, e2;
    dn::DeviceBuffer<uint8_t> d_comp, d_out;
    dn::DeviceBuffer<dn::InflateBlock> d_blk;
    dn::DeviceBuffer<int32_t> d_status;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate)); DN_TRY(e1.create(hipEventCreate)); DN_TRY(e2.create(hipEventCreate));
        DN_TRY(d_comp.alloc((size_t) cap));
        DN_TRY(d_out.alloc((size_t) n_out + 16));
        DN_TRY(d_blk.alloc(sizeof(dn::InflateBlock) * (size_t) n_blocks));
        DN_TRY(d_status.alloc(sizeof(int32_t) * (size_t) n_blocks));
        DN_TRY(hipEventRecord(e0, st));
        if (n_comp > 0) DN_TRY(hipMemcpyAsync(d_comp, comp, (size_t) n_comp, hipMemcpyHostToDevice, st));
        DN_TRY(hipMemcpyAsync(d_blk, blk.data(), sizeof(dn::InflateBlock) * (size_t) n_blocks, hipMemcpyHostToDevice, st));
        DN_TRY(hipEventRecord(e1, st));
        DN_TRY(dn::inflate_launch(st, d_comp, cap, d_blk, n_blocks, d_out, d_status));
        DN_TRY(hipEventRecord(e2, st));
        if (n_out > 0) DN_TRY(hipMemcpyAsync(out, d_out, (size_t) n_out, hipMemcpyDeviceToHost, st));
        DN_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t) n_blocks, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        float ms = 0.f;
        if (copy_ms) { DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *copy_ms = ms; }
        if (device_ms) { DN_TRY(hipEventElapsedTime(&ms, e1, e2)); *device_ms = ms; }
        return DN_OK;
    });
}

}  // namespace

hipError_t dn::inflate_launch(hipStream_t st, const uint8_t *d_comp, int64_t comp_cap, const InflateBlock *d_blk, int64_t n_blocks,
                              uint8_t *d_out, int32_t *d_status)
{
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned) n_blocks), dim3(64), 0, st, d_comp, comp_cap, d_blk, n_blocks, d_out, d_status);
    return hipGetLastError();
}

int dn::InflateWindow::arm(const char *who, const uint32_t *crc32, int64_t n_blocks)
{
    if (n_blocks < 0 || n_blocks > INT32_MAX || (n_blocks > 0 && !crc32)) return bad(std::string(who) + ": bad argument");
    announced.assign(crc32, crc32 + n_blocks);
    armed = true;
    return DN_OK;
}

int dn::InflateWindow::plan(const char *who, const char *armed_by, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                            const int32_t *pay_len, const int32_t *isize, int32_t head_skip, int32_t tail_keep, int64_t base, int64_t &total)
{
    const std::string w(who);
    if (checking && (int64_t) crc.size() != n_blocks)
        return bad(w + ": " + std::to_string(crc.size()) + " CRC32s were announced (" + armed_by + ") for " + std::to_string(n_blocks) + " blocks");
    blk.resize((size_t) n_blocks);
    total = base;
    for (int64_t b = 0; b < n_blocks; b++) {
        if (isize[b] < 0) return bad(w + ": block " + std::to_string(b) + " has a negative inflated size");
        if (!payload_inside(pay_off[b], pay_len[b], n_comp)) return bad(w + ": payload of block " + std::to_string(b) + " outside comp");
        int32_t skip, keep;
        window_trim(b, n_blocks, isize[b], head_skip, tail_keep, skip, keep);
        blk[(size_t) b] = InflateBlock{pay_off[b], total, pay_len[b], isize[b], skip, keep, checking ? crc[(size_t) b] : 0u, checking ? 1 : 0};
        total += keep;
    }
    return DN_OK;
}

int dn::InflateWindow::queue(hipStream_t st, const uint8_t *comp_bytes, int64_t n_comp, uint8_t *d_out, int32_t *status)
{
    const int64_t n_blocks = (int64_t) blk.size(), comp_cap = inflate_comp_cap(n_comp);
    DN_TRY(comp.reserve(comp_cap, 0, st));
    DN_TRY(d_blk.reserve(n_blocks, 0, st)); DN_TRY(d_status.reserve(n_blocks, 0, st));
    if (!ev0) { DN_TRY(ev0.create(hipEventCreate)); DN_TRY(ev1.create(hipEventCreate)); }
    if (n_comp > 0) DN_TRY(hipMemcpyAsync(comp, comp_bytes, (size_t) n_comp, hipMemcpyHostToDevice, st));
    if (n_blocks > 0) DN_TRY(hipMemcpyAsync(d_blk, blk.data(), sizeof(InflateBlock) * (size_t) n_blocks, hipMemcpyHostToDevice, st));
    DN_TRY(hipEventRecord(ev0, st));
    DN_TRY(inflate_launch(st, comp, comp_cap, d_blk, n_blocks, d_out, d_status));
    DN_TRY(hipEventRecord(ev1, st));
    if (n_blocks > 0) DN_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t) n_blocks, hipMemcpyDeviceToHost, st));
    return DN_OK;
}

int dn::InflateWindow::wait(hipStream_t st, const int32_t *status, double *ms, bool &ok)
{
    DN_TRY(hipStreamSynchronize(st));
    if (ms) {
        float t = 0.f;
        DN_TRY(hipEventElapsedTime(&t, ev0, ev1));
        *ms = t;
    }
    ok = true;
    for (size_t b = 0; b < blk.size(); b++) ok = ok && status[b] == 0;
    return DN_OK;
}

extern "C" int dn_bgzf_inflate_host(const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                                    const int64_t *out_off, uint8_t *out, int32_t *status)
{
    return inflate_host("dn_bgzf_inflate_host", comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, false, status, nullptr);
}

extern "C" int dn_bgzf_inflate_check_host(const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                                          const int64_t *out_off, uint8_t *out, int32_t *status, const uint32_t *crc32)
{
    return inflate_host("dn_bgzf_inflate_check_host", comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, true, status, crc32);
}

extern "C" int dn_bgzf_inflate(int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                               const int32_t *pay_len, const int64_t *out_off, uint8_t *out, int32_t *status, double *copy_ms,
                               double *device_ms)
{
    return inflate_device("dn_bgzf_inflate", device, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, false, status, copy_ms, device_ms,
                          nullptr);
}

extern "C" int dn_bgzf_inflate_check(int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                                     const int32_t *pay_len, const int64_t *out_off, uint8_t *out, int32_t *status, double *copy_ms,
                                     double *device_ms, const uint32_t *crc32)
{
    return inflate_device("dn_bgzf_inflate_check", device, comp, n_comp, n_blocks, pay_off, pay_len, out_off, out, true, status, copy_ms,
                          device_ms, crc32);
}

extern "C" int dn_bgzf_crc32_host(const uint8_t *data, int64_t n, int32_t lanes, int32_t flush_bytes, uint32_t *crc)
{
    dn::clear_error();
    if (n < 0 || (n > 0 && !data) || lanes < 1 || lanes > 64 || flush_bytes < 1 || flush_bytes > (1 << 30) || !crc)
        return bad("dn_bgzf_crc32_host: bad argument (lanes is 1 .. 64, flush_bytes 1 .. 2^30)");
    *crc = crc_host(0xffffffffu, data, n, lanes, flush_bytes) ^ 0xffffffffu;
    return DN_OK;
}

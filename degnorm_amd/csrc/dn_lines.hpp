// dn_lines.hpp -- the lines of a text window on the device: what the GTF scanner (dn_gtf.hip), the GFF3 scanner
// (dn_gff3.hip) and the SAM encoder (dn_sam.hip) share.  Each has a window of text that ends at a line end in a buffer
// zero-padded to whole 16 KiB tiles (upload_padded; the GFF3 handle keeps one such buffer for the file) and finds where every
// line starts in three passes, which LineTable owns and runs:
//   k_count_newlines   '\n' per 16 KiB tile (four 16-byte loads per lane)
//   k_scan             exclusive prefix sum of the tile counts (one workgroup)
//   k_line_starts      the byte offset every line starts at
// Then one lane takes one line (line_span) and reads it through Bytes: aligned 8-byte words of the padded buffer, and only
// at positions below the line's end, which is at most the bytes uploaded.  The first faulty line of a window in file order
// is found by atomicMin on one word (report_error, unpack_error).
// Everything lives in the unnamed namespace: every unit that includes this header compiles its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "dn_host.hpp"

namespace {

constexpr int kNT = 256;
constexpr int kLaneBytes = 64;                      // bytes of a tile one lane counts: four 16-byte loads
constexpr int64_t kTile = (int64_t) kNT * kLaneBytes;
constexpr int kScanNT = 1024;

__device__ inline int newlines16(const uint4 v)
{
    int n = 0;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t x = w[k] ^ 0x0a0a0a0au;                               // a zero byte where the word holds '\n'
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 in exactly those bytes
        n += __popc(z);
    }
    return n;
}

// exclusive prefix sum of one value per lane over the workgroup (kNT lanes); *total: the sum
__device__ inline int block_exclusive(int v, int *total)
{
    __shared__ int s[kNT];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < kNT; d <<= 1) {
        const int add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[kNT - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kNT) void k_count_newlines(const uint4 *__restrict__ buf, int64_t n_tiles, int32_t *__restrict__ tile_count)
{
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint4 *p = buf + (tile * kTile + (int64_t) threadIdx.x * kLaneBytes) / 16;
        const int n = newlines16(p[0]) + newlines16(p[1]) + newlines16(p[2]) + newlines16(p[3]);
        int total;
        (void) block_exclusive(n, &total);
        if (threadIdx.x == 0) tile_count[tile] = total;
    }
}

// out[i] = in[0] + ... + in[i - 1], *total = the sum of all n; one workgroup, lane t takes the t-th contiguous share
__global__ __launch_bounds__(kScanNT) void k_scan(const int32_t *__restrict__ in, int64_t n, int64_t *__restrict__ out, int64_t *__restrict__ total)
{
    __shared__ int64_t s[kScanNT];
    const int t = threadIdx.x;
    const int64_t share = (n + kScanNT - 1) / kScanNT;
    const int64_t lo = t * share < n ? t * share : n, hi = lo + share < n ? lo + share : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; i++) sum += in[i];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanNT; d <<= 1) {
        const int64_t add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    int64_t run = s[t] - sum;
    for (int64_t i = lo; i < hi; i++) { out[i] = run; run += in[i]; }
    if (t == kScanNT - 1) *total = s[t];
}

// line_start[0] = 0 (set by the host code), line_start[k] = 1 + the position of the k-th '\n'; n_starts entries
__global__ __launch_bounds__(kNT) void k_line_starts(const uint8_t *__restrict__ buf, int64_t n_tiles, const int64_t *__restrict__ tile_off,
                                                      int64_t *__restrict__ line_start, int64_t n_starts)
{
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * kTile + (int64_t) threadIdx.x * kLaneBytes;
        const uint4 *p = (const uint4 *) (buf + base);
        uint4 v[4] = {p[0], p[1], p[2], p[3]};
        const int n = newlines16(v[0]) + newlines16(v[1]) + newlines16(v[2]) + newlines16(v[3]);
        int total;
        int64_t k = tile_off[tile] + block_exclusive(n, &total) + 1;
        if (n == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (((w[b >> 2] >> (8 * (b & 3))) & 0xffu) == 0x0au) {
                    if (k < n_starts) line_start[k] = base + 16 * j + b + 1;
                    k++;
                }
        }
    }
}

// byte reads through aligned 8-byte words; the buffer is padded to whole tiles, so the word of any position below n_bytes
// lies inside the allocation
struct Bytes {
    const uint64_t *w;
    int64_t idx;
    uint64_t cur;
    __device__ explicit Bytes(const uint8_t *buf) : w((const uint64_t *) buf), idx(-1), cur(0) {}
    __device__ uint32_t at(int64_t pos)
    {
        const int64_t i = pos >> 3;
        if (i != idx) { idx = i; cur = w[i]; }
        return (uint32_t) (cur >> (8 * (pos & 7))) & 0xffu;
    }
};

inline unsigned grid_capped(int64_t n) { return (unsigned) (n < 1 ? 1 : n > 2048 ? 2048 : n); }

// the line i: [*beg, *end) without its '\n'; the last of the n_starts lines ends at `limit`
__device__ inline void line_span(const int64_t *__restrict__ line_start, int64_t n_starts, int64_t limit, int64_t i, int64_t *beg, int64_t *end)
{
    *beg = line_start[i];
    *end = i + 1 < n_starts ? line_start[i + 1] - 1 : limit;
}

// The first faulty line of a call: one word, the line above the kind's eight bits, that starts as kNoError and takes the
// smallest report.
constexpr unsigned long long kNoError = ~0ull;

__device__ inline void report_error(unsigned long long *first_error, int64_t line, int kind)
{
    atomicMin(first_error, ((unsigned long long) line << 8) | (unsigned long long) kind);
}

// true, *err_line and *err_kind: the word holds a report
inline bool unpack_error(unsigned long long word, int64_t *err_line, int32_t *err_kind)
{
    if (word == kNoError) return false;
    *err_line = (int64_t) (word >> 8);
    *err_kind = (int32_t) (word & 0xffu);
    return true;
}

// '\n' among the n bytes at p, on the host
inline int64_t count_newlines(const uint8_t *p, int64_t n)
{
    int64_t k = 0;
    for (const uint8_t *e = p + n; (p = (const uint8_t *) memchr(p, '\n', (size_t) (e - p))) != nullptr; p++) k++;
    return k;
}

// n_bytes of the caller's text to a device buffer of `padded` bytes (whole tiles), zeros behind them
inline hipError_t upload_padded(hipStream_t st, uint8_t *dst, const uint8_t *src, int64_t n_bytes, int64_t padded)
{
    const hipError_t e = hipMemcpyAsync(dst, src, (size_t) n_bytes, hipMemcpyHostToDevice, st);
    return e == hipSuccess && padded > n_bytes ? hipMemsetAsync(dst + n_bytes, 0, (size_t) (padded - n_bytes), st) : e;
}

// Where the lines of n_tiles tiles start.  Declared in the frame that calls dn::synced (dn_host.hpp): the stream writes
// n_newlines.  `total` is free for the caller's own k_scan calls once find has returned.
struct LineTable {
    dn::DeviceBuffer<int32_t> tile_count;
    dn::DeviceBuffer<int64_t> tile_off, total, line_start;
    int64_t n_newlines = 0;
    int64_t n_starts = 0;               // n_newlines + 1: the last one starts an empty line when the bytes end in '\n'

    hipError_t alloc(int64_t n_tiles)
    {
        hipError_t e = tile_count.alloc(sizeof(int32_t) * (size_t) n_tiles);
        if (e == hipSuccess) e = tile_off.alloc(sizeof(int64_t) * (size_t) n_tiles);
        if (e == hipSuccess) e = total.alloc(sizeof(int64_t));
        return e;
    }

    // Counts the '\n' of the tiles (after alloc), waits for the count -- the one synchronisation --, holds it to [lo, hi] and
    // queues k_line_starts into a line_start of n_starts entries.  The DN_* code; `entry` names the caller in the error text.
    int find(hipStream_t st, const uint8_t *tiles, int64_t n_tiles, int64_t lo, int64_t hi, const char *entry)
    {
        hipLaunchKernelGGL(k_count_newlines, dim3(grid_capped(n_tiles)), dim3(kNT), 0, st, (const uint4 *) tiles, n_tiles, tile_count.get());
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanNT), 0, st, tile_count.get(), n_tiles, tile_off.get(), total.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&n_newlines, total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (n_newlines < lo || n_newlines > hi) return dn::fail(DN_E_STATE, std::string(entry) + ": newline count out of range");
        n_starts = n_newlines + 1;
        DN_TRY(line_start.alloc(sizeof(int64_t) * (size_t) n_starts));
        DN_TRY(hipMemsetAsync(line_start, 0, sizeof(int64_t), st));
        hipLaunchKernelGGL(k_line_starts, dim3(grid_capped(n_tiles)), dim3(kNT), 0, st, tiles, n_tiles, (const int64_t *) tile_off.get(),
                           line_start.get(), n_starts);
        return DN_OK;
    }
};

}  // namespace

// dn_deflate.hpp -- what the sort unit (dn_sort.hip) needs of the BGZF deflate unit (dn_deflate.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "dn_host.hpp"

namespace dn {

constexpr int32_t kDeflateMaxLen = 0xff00;      // input bytes of one BGZF block
constexpr int64_t kDeflateSlot = 65536;         // bytes of device memory a block is written into before the compaction
// device bytes one block needs of the region handed to deflate_device: its slot and its share of the compacted output
constexpr int64_t kDeflateRegionPerBlock = 2 * kDeflateSlot;

// the largest BGZF block `len` input bytes can become (include/degnorm_amd.h, dn_bgzf_deflate_bound); -1 for a bad length
int64_t deflate_bound(int64_t len);

// DN_OK, or DN_E_INVALID with the error text set: the checks dn_bgzf_deflate and dn_bgzf_deflate_host make before any work
int deflate_validate(const char *who, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, const uint8_t *out,
                     int64_t out_cap, const int64_t *out_off);

// the small device tables of deflate_device, kept between calls
struct DeflateTables {
    GrowBuffer<int64_t> beg, off;
    GrowBuffer<int32_t> len, size;
    Event e0, e1;
    std::vector<int32_t> h_size;
    std::vector<int64_t> h_off;
};

// The blocks data[beg[b] .. beg[b] + len[b]) of device memory d_data (16-byte aligned, readable up to the next multiple of
// four behind the last range) -> whole BGZF blocks, back to back in out (host memory), block b at out_off[b]; out_off[n_blocks]
// is their size.  `region` is device memory of region_bytes (at least kDeflateRegionPerBlock, 16-byte aligned) the call may
// overwrite: batches of region_bytes / kDeflateRegionPerBlock blocks are deflated into slots, compacted and copied to out.
// The arguments were validated.  *ms (nullable) gains the device time of the kernels.  Waits for st before it returns DN_OK.
int deflate_device(hipStream_t st, const uint8_t *d_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *region,
                   int64_t region_bytes, DeflateTables &t, uint8_t *out, int64_t *out_off, double *ms);

// the same by the host build, on host memory
int deflate_host(const uint8_t *data, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *out, int64_t *out_off);

}  // namespace dn

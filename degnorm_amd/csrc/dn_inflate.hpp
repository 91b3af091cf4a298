// dn_inflate.hpp -- what the reads unit (dn_reads.hip) needs of the BGZF inflate unit (dn_inflate.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace dn

// dn_gz.hpp -- the records that the gzip unit (dn_gz.hip) passes between its host code and its kernels.  Bit offsets are
// relative to the first byte of the span that is on the device (include/degnorm_amd.h, "gzip streams").
#pragma once
#include <stdint.h>

namespace dn {
namespace gz {

constexpr int kHistory = 32768;              // DEFLATE's reach: symbols in a tail, bytes in a window

// what a walk leaves: status 0 or DN_INFLATE_E_*, -1 for a chunk without a guess (nothing walked)
struct Segment {
    int64_t entry, exit, out_len;
    int32_t kind, blocks, status, pad;
};

// a fix-up walk: from `entry` to the first block end that is a guess; its tail goes to slot `slot`
struct Unit {
    int64_t entry;
    int64_t slot;
};

// one segment of the chain for the window and emit passes: bits [entry, exit) inflate to out_len bytes at out_off; the
// tail of its walk is in slot `slot`; reset: the first segment of a member (window all zero, have = 0)
struct Emit {
    int64_t entry, exit, out_off, out_len;
    int32_t have, slot, reset, kind;
};

struct EmitResult {
    uint32_t crc;                            // the register after the segment's bytes, started from 0
    int32_t status;
};

}  // namespace gz
}  // namespace dn

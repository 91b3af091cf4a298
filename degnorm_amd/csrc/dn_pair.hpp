// dn_pair.hpp -- pairing the mates of paired-end reads: the rows of a store in ascending qname_unpaired order, and the
// id of every row's key in that order.
//
// A key is row r's bytes names[name_beg[r] .. name_beg[r] + key_len[r]).  Keys compare as unsigned bytes, zero-padded to
// the longest of them (so a key that is a prefix of another comes first), and rows of equal key stay in ascending row
// order: np.argsort(keys, kind='stable') on the fixed-width keys of dn_bam_rows_keys.  The sort is an LSD radix sort over
// 8-byte chunks of the key, last chunk first: pair_chunk reads a chunk straight from the names, big-endian into a
// uint64_t with zero past the key's end, and a stable sort of (chunk, row) follows -- hipcub's on the device,
// std::stable_sort in the host entry.  pair_same_key then compares every row with its predecessor in the final order.
// Both are __host__ __device__: the host entry runs what the kernels run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dn_host.hpp"

namespace dn {

constexpr int kPairChunk = 8;                   // key bytes a pass sorts by

// passes over keys of at most max_key bytes (0: every key is empty, and file order is the order)
inline int pair_passes(int32_t max_key) { return (max_key + kPairChunk - 1) / kPairChunk; }

// chunk c of the key of `len` bytes at names + beg.  Reads no byte at or past beg + len.
__host__ __device__ __forceinline__ uint64_t pair_chunk(const uint8_t *names, int64_t beg, int32_t len, int32_t c)
{
    uint64_t v = 0;
    const int32_t o = c * kPairChunk;
    for (int k = 0; k < kPairChunk; k++) v = (v << 8) | (o + k < len ? (uint64_t) names[beg + o + k] : 0);
    return v;
}

// whether two keys are equal once zero-padded to the longer one: what the sort treats as one key
__host__ __device__ __forceinline__ bool pair_same_key(const uint8_t *names, int64_t beg_a, int32_t len_a, int64_t beg_b, int32_t len_b)
{
    const int32_t shorter = len_a < len_b ? len_a : len_b, longer = len_a < len_b ? len_b : len_a;
    const int64_t rest = len_a < len_b ? beg_b : beg_a;
    for (int32_t k = 0; k < shorter; k++)
        if (names[beg_a + k] != names[beg_b + k]) return false;
    for (int32_t k = shorter; k < longer; k++)
        if (names[rest + k] != 0) return false;
    return true;
}

// Pairing by FLAG (the rule: include/degnorm_amd.h).  A row's key is then its whole name and the two mate coordinates,
// which these arrays give; pos == NULL is the name rule above.  The coordinates are one more chunk below the name's:
// mate_chunk, sorted before every name chunk, so rows go by name, then (uint32) (pos_first + 1), then
// (uint32) (pos_last + 1).  A row with 0x40 set is a first mate: pos_first is its pos and pos_last its next_pos; any
// other row has them the other way round.
struct MateCoords {
    const int64_t *pos = nullptr;
    const int32_t *next_pos = nullptr;
    const uint16_t *flag = nullptr;
};

constexpr uint32_t kFlagFirst = 0x40, kFlagLast = 0x80;

__host__ __device__ __forceinline__ uint64_t mate_chunk(int64_t pos, int32_t next_pos, uint32_t flag)
{
    const uint32_t p = (uint32_t) pos + 1u, q = (uint32_t) next_pos + 1u;           // -1 (no position) sorts first
    return (flag & kFlagFirst) ? (uint64_t) p << 32 | q : (uint64_t) q << 32 | p;
}

// What pair_device needs besides its outputs: two (uint64, int32) arrays of n and the radix sort's workspace.  Declared
// by the frame that waits for the stream.
struct PairWork {
    DeviceBuffer<uint64_t> ka, kb;
    DeviceBuffer<int32_t> oa, ob;
    Scratch scratch;
};

// Queue the pairing of n rows (0 < n < 2^31) with keys of at most max_key bytes on st: order[n] and pair_id[n], device
// arrays.  The number of ids is pair_id[n - 1] + 1.  mates.pos != NULL: the keys end in the rows' mate_chunk.  A DN_* code.
int pair_device(hipStream_t st, int64_t n, int32_t max_key, const int64_t *name_beg, const int32_t *key_len, const uint8_t *names,
                const MateCoords &mates, PairWork &W, int32_t *order, int32_t *pair_id);

}  // namespace dn

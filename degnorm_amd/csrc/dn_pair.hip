// dn_pair.hip -- the mates of paired-end reads, paired on the device (dn_pair.hpp: the order and its two per-row steps).
//
//   k_pair_chunk   one lane per row: the pass's chunk of every row in the current order (file order before the first pass)
//   k_pair_mates   (pairing by FLAG) the same for the chunk of the two mate coordinates, the first pass of all, over 64 bits
//   sort           hipcub::DeviceRadixSort::SortPairs of (chunk, row), which is stable; the last chunk, sorted first, only
//                  over the bits its bytes can set.  Those bytes are moved to the low end of the word and the sort runs
//                  over bits [0, 8 * bytes): a range that ends at bit 64 without starting at bit 0 is not sorted by the
//                  merge-sort path rocPRIM takes for 1 025 rows up to its merge_sort_limit, whose comparator builds its
//                  mask with a shift by 64
//   k_pair_heads   one lane per row: the final order, and 1 where a row's key differs from its predecessor's (MATES: the
//                  coordinate chunk is part of the key)
//   scan           inclusive sum of those flags, in place: the pair ids
//
// Extra device memory is linear in the rows: two (uint64, int32) arrays and hipcub's workspace; no array of padded keys.
// dn_bam_pair_host and dn_bam_mate_host run the same passes on host arrays, with std::stable_sort in place of the radix sort.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_bam_record.hpp"
#include "dn_pair.hpp"

namespace {

constexpr int kNT = 256;
constexpr int64_t kGridCap = 65536;

// low bits of the chunk of pass c that no key of at most max_key bytes can set
inline int pair_unset_bits(int32_t max_key, int c)
{
    const int sig = max_key - c * dn::kPairChunk;
    return sig >= dn::kPairChunk ? 0 : 8 * (dn::kPairChunk - sig);
}

__global__ __launch_bounds__(kNT) void k_pair_chunk(int64_t n, const int32_t *__restrict__ cur, const int64_t *__restrict__ name_beg,
                                                    const int32_t *__restrict__ key_len, const uint8_t *__restrict__ names, int32_t c,
                                                    int32_t shift, uint64_t *__restrict__ chunk, int32_t *__restrict__ row)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) {
        const int32_t s = cur ? cur[i] : (int32_t) i;
        chunk[i] = dn::pair_chunk(names, name_beg[s], key_len[s], c) >> shift;
        row[i] = s;
    }
}

__global__ __launch_bounds__(kNT) void k_pair_mates(int64_t n, dn::MateCoords M, uint64_t *__restrict__ chunk, int32_t *__restrict__ row)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) {
        chunk[i] = dn::mate_chunk(M.pos[i], M.next_pos[i], M.flag[i]);
        row[i] = (int32_t) i;
    }
}

template <bool MATES>
__global__ __launch_bounds__(kNT) void k_pair_heads(int64_t n, const int32_t *__restrict__ cur, const int64_t *__restrict__ name_beg,
                                                    const int32_t *__restrict__ key_len, const uint8_t *__restrict__ names, dn::MateCoords M,
                                                    int32_t *__restrict__ order, int32_t *__restrict__ head)
{
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t) gridDim.x * kNT) {
        const int32_t s = cur ? cur[i] : (int32_t) i;
        int32_t f = 0;
        if (i > 0) {
            const int32_t p = cur ? cur[i - 1] : (int32_t) (i - 1);
            f = !dn::pair_same_key(names, name_beg[s], key_len[s], name_beg[p], key_len[p]);
            if (MATES) f |= dn::mate_chunk(M.pos[s], M.next_pos[s], M.flag[s]) != dn::mate_chunk(M.pos[p], M.next_pos[p], M.flag[p]);
        }
        order[i] = s;
        head[i] = f;
    }
}

}  // namespace

int dn::pair_device(hipStream_t st, int64_t n, int32_t max_key, const int64_t *name_beg, const int32_t *key_len, const uint8_t *names,
                    const MateCoords &mates, PairWork &W, int32_t *order, int32_t *pair_id)
{
    const bool by_flag = mates.pos != nullptr;
    if (n < 1 || n > INT32_MAX || max_key < 0 || !name_beg || !key_len || !order || !pair_id || (by_flag && (!mates.next_pos || !mates.flag)))
        return dn::fail(DN_E_INVALID, "pair_device: bad argument");
    const int passes = pair_passes(max_key);
    const dim3 grid(dn::grid_for(n, kNT, kGridCap)), block(kNT);
    const int32_t *cur = nullptr;                    // the order so far: file order
    if (passes > 0 || by_flag) {
        DN_TRY(alloc_padded(W.ka, (size_t) n)); DN_TRY(alloc_padded(W.kb, (size_t) n));
        DN_TRY(alloc_padded(W.oa, (size_t) n)); DN_TRY(alloc_padded(W.ob, (size_t) n));
    }
    if (by_flag) {                                   // the least significant chunk: the mate coordinates
        hipLaunchKernelGGL(k_pair_mates, grid, block, 0, st, n, mates, W.ka.get(), W.oa.get());
        DN_TRY(hipGetLastError());
        DN_TRY(W.scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint64_t *) W.ka.get(), W.kb.get(), (const int32_t *) W.oa.get(), W.ob.get(),
                                                      (int) n, 0, 64, st);
        }));
        cur = W.ob;
    }
    for (int c = passes - 1; c >= 0; c--) {
        const int shift = pair_unset_bits(max_key, c);
        hipLaunchKernelGGL(k_pair_chunk, grid, block, 0, st, n, cur, name_beg, key_len, names, (int32_t) c, (int32_t) shift, W.ka.get(), W.oa.get());
        DN_TRY(hipGetLastError());
        DN_TRY(W.scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint64_t *) W.ka.get(), W.kb.get(), (const int32_t *) W.oa.get(), W.ob.get(),
                                                      (int) n, 0, 64 - shift, st);
        }));
        cur = W.ob;
    }
    if (by_flag) hipLaunchKernelGGL(k_pair_heads<true>, grid, block, 0, st, n, cur, name_beg, key_len, names, mates, order, pair_id);
    else hipLaunchKernelGGL(k_pair_heads<false>, grid, block, 0, st, n, cur, name_beg, key_len, names, mates, order, pair_id);
    DN_TRY(hipGetLastError());
    DN_TRY(W.scratch.run([&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::InclusiveSum(tmp, bytes, pair_id, pair_id, (int) n, st); }));
    return DN_OK;
}

namespace {

// the passes of pair_device on host arrays; mates: as there
int pair_host(const char *who, int64_t n, const int64_t *name_beg, const int32_t *key_len, const uint8_t *names, const dn::MateCoords &mates,
              int32_t *order, int32_t *pair_id, int64_t *n_pair_ids)
{
    const bool by_flag = mates.pos != nullptr;
    if (n < 0 || n > INT32_MAX || !n_pair_ids || (n > 0 && (!name_beg || !key_len || !order || !pair_id)) ||
        (n > 0 && by_flag && (!mates.next_pos || !mates.flag)))
        return dn::fail(DN_E_INVALID, std::string(who) + ": bad argument");
    *n_pair_ids = 0;
    if (n == 0) return DN_OK;
    int32_t max_key = 0;
    for (int64_t r = 0; r < n; r++) {
        if (key_len[r] < 0 || name_beg[r] < 0 || (key_len[r] > 0 && !names)) return dn::fail(DN_E_INVALID, std::string(who) + ": bad key");
        max_key = std::max(max_key, key_len[r]);
    }
    std::vector<std::pair<uint64_t, int32_t>> v((size_t) n);
    const auto sort_pass = [&]() {
        std::stable_sort(v.begin(), v.end(), [](const std::pair<uint64_t, int32_t> &a, const std::pair<uint64_t, int32_t> &b) { return a.first < b.first; });
        for (int64_t i = 0; i < n; i++) order[i] = v[(size_t) i].second;
    };
    const auto mate_of = [&](int32_t r) { return dn::mate_chunk(mates.pos[r], mates.next_pos[r], mates.flag[r]); };
    for (int64_t i = 0; i < n; i++) order[i] = (int32_t) i;
    if (by_flag) {
        for (int64_t i = 0; i < n; i++) v[(size_t) i] = {mate_of((int32_t) i), (int32_t) i};
        sort_pass();
    }
    for (int c = dn::pair_passes(max_key) - 1; c >= 0; c--) {
        for (int64_t i = 0; i < n; i++) v[(size_t) i] = {dn::pair_chunk(names, name_beg[order[i]], key_len[order[i]], c), order[i]};
        sort_pass();
    }
    pair_id[0] = 0;
    for (int64_t i = 1; i < n; i++) {
        const int32_t s = order[i], p = order[i - 1];
        bool differ = !dn::pair_same_key(names, name_beg[s], key_len[s], name_beg[p], key_len[p]);
        if (by_flag) differ |= mate_of(s) != mate_of(p);
        pair_id[i] = pair_id[i - 1] + differ;
    }
    *n_pair_ids = (int64_t) pair_id[n - 1] + 1;
    return DN_OK;
}

}  // namespace

extern "C" int dn_bam_pair_host(int64_t n, const int64_t *name_beg, const int32_t *key_len, const uint8_t *names, int32_t *order,
                                int32_t *pair_id, int64_t *n_pair_ids)
{
    dn::clear_error();
    return pair_host("dn_bam_pair_host", n, name_beg, key_len, names, dn::MateCoords{}, order, pair_id, n_pair_ids);
}

extern "C" int dn_bam_mate_host(int64_t n, const int64_t *name_beg, const int32_t *name_len, const uint8_t *names, const int64_t *pos,
                                const int32_t *next_pos, const uint16_t *flag, int32_t *order, int32_t *pair_id, int64_t *n_pair_ids)
{
    dn::clear_error();
    if (n > 0 && !pos) return dn::fail(DN_E_INVALID, "dn_bam_mate_host: bad argument");
    static const int64_t no_pos = 0;                 // n == 0: the rule is still the FLAG rule
    dn::MateCoords M;
    M.pos = pos ? pos : &no_pos; M.next_pos = next_pos; M.flag = flag;
    return pair_host("dn_bam_mate_host", n, name_beg, name_len, names, M, order, pair_id, n_pair_ids);
}

// dn_bam_record.hpp -- what a BAM record is, for the units that read inflated records (dn_frame.hip, dn_reads.hip,
// dn_bai.hip, dn_sort.hip) and the one that writes them (dn_sam.hip): little-endian readers, the fixed part of a record
// as a view with its shape checks, the key that sorts a refID, the bin of a range, the launch grid of a per-record kernel
// -- and, for the index and the sort, the rule "the first faulty record in file order wins" with the texts that name a
// record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "dn_host.hpp"

#define DN_HD __host__ __device__ __forceinline__

namespace dn {

// Byte loads, because record fields sit at arbitrary offsets.
DN_HD uint32_t le16(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }
DN_HD uint32_t le32(const uint8_t *p)
{
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

// Where the fixed fields lie, from the first byte of block_size (SAM specification 4.2).  block_size counts what follows
// it: kBamMinSize bytes of fixed fields, then read name, CIGAR, sequence, qualities and aux fields.
enum : int {
    kBamRef = 4, kBamPos = 8, kBamLName = 12, kBamNCigar = 16, kBamFlag = 18, kBamLSeq = 20, kBamNextRef = 24, kBamNextPos = 28,
    kBamName = 36,                      // the end of the fixed part
    kBamPosEnd = 12,                    // block_size, refID and pos: what a text that names a record reads
    kBamMinSize = 32
};

// the fixed part of the record at byte o of a window
struct BamHead {
    int64_t o;
    int32_t bs, ref, pos, l_seq, next_ref, next_pos;
    uint32_t l_name, n_cig, flag;

    DN_HD int64_t name() const { return o + kBamName; }
    DN_HD int64_t cigar() const { return name() + l_name; }
    DN_HD int64_t end() const { return o + 4 + bs; }
    // read name and CIGAR lie inside the record
    DN_HD bool names_fit() const { return kBamMinSize + (int64_t) l_name + 4 * (int64_t) n_cig <= bs; }
};

// Fill H from the record at w[o ..); false when its fixed part or its block_size bytes do not lie inside the n_bytes of w,
// or block_size is below 32.  Everything is inlined, so a caller pays for the loads of the fields it uses.
DN_HD bool bam_head(const uint8_t *w, int64_t n_bytes, int64_t o, BamHead &H)
{
    if (o < 0 || o + kBamName > n_bytes) return false;
    H.o = o;
    H.bs = (int32_t) le32(w + o);
    if (H.bs < kBamMinSize || o + 4 + (int64_t) H.bs > n_bytes) return false;
    H.ref = (int32_t) le32(w + o + kBamRef);
    H.pos = (int32_t) le32(w + o + kBamPos);
    H.l_name = w[o + kBamLName];
    H.n_cig = le16(w + o + kBamNCigar);
    H.flag = le16(w + o + kBamFlag);
    H.l_seq = (int32_t) le32(w + o + kBamLSeq);
    H.next_ref = (int32_t) le32(w + o + kBamNextRef);
    H.next_pos = (int32_t) le32(w + o + kBamNextPos);
    return true;
}

// The 32-bit value that orders references: refID -1 maps to the largest, so unplaced records sort last.
constexpr uint32_t kUnplaced = 0xffffffffu;
DN_HD uint32_t ref_key(int32_t ref) { return ref < 0 ? kUnplaced : (uint32_t) ref; }

// The bin of [beg, end) on a reference (SAM specification 5.3), which holds for 0 <= beg < end <= 2^29.  The SAM encoder
// (dn_sam.hip) calls it with any beg >= -1: the shifts are arithmetic, so beg = -1, end = 0 gives 4680.
DN_HD uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t) (((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t) (((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t) (((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t) (((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t) (((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// The same for a binning scheme of `depth` levels below the root whose smallest bins span 2^min_shift bases (the .csi
// index; (14, 5) is the function above), with 0 <= beg < end <= 2^(min_shift + 3 depth), min_shift + 3 depth <= 54, depth <= 8.
DN_HD uint32_t reg2bin(int64_t beg, int64_t end, int min_shift, int depth)
{
    int l = depth, s = min_shift;
    uint32_t t = (((uint32_t) 1 << 3 * depth) - 1) / 7;
    --end;
    while (l > 0) {
        if (beg >> s == end >> s) return t + (uint32_t) (beg >> s);
        --l; s += 3; t -= (uint32_t) 1 << 3 * l;
    }
    return 0;
}

// Strand-specific counting (include/degnorm_amd.h): the strand the fragment of a row came from, '+' or '-'.  A row is a last
// mate when FLAG 0x1 and 0x80 are both set, and in a store paired by the name rule (by_name) also when its name ends in '2'
// (name_last: the last byte of the name, 0 for an empty one).  The sense is the strand the row aligned to (0x10: '-'),
// flipped for a last mate and flipped once more for the protocol kStrandReverse.
enum : int { kStrandNo = 0, kStrandForward = 1, kStrandReverse = 2 };
constexpr uint8_t kSensePlus = '+', kSenseMinus = '-';

DN_HD uint8_t row_sense(uint32_t flag, uint8_t name_last, bool by_name, int protocol)
{
    const bool last_mate = (flag & 0x81u) == 0x81u || (by_name && name_last == '2');
    const bool minus = ((flag & 0x10u) != 0) != last_mate;
    return (minus != (protocol == kStrandReverse)) ? kSenseMinus : kSensePlus;
}

// blocks of a grid-stride kernel that gives each block per_block of the n items, at most cap
inline unsigned grid_for(int64_t n, int per_block, int64_t cap)
{
    const int64_t g = (n + per_block - 1) / per_block;
    return (unsigned) (g < 1 ? 1 : g > cap ? cap : g);
}

// ---- the first faulty record in file order wins ---------------------------------------------------------------------
// A pass over records notes (ordinal, code) of every faulty one, code in 1 .. 7, in one 64-bit word preset to kNoError;
// the smallest ordinal << 3 | code stays: the first faulty record, whatever its code.

constexpr unsigned long long kNoError = ~0ull;

DN_HD void note_error(unsigned long long *word, int64_t ordinal, int code)
{
    const unsigned long long v = (unsigned long long) ordinal << 3 | (unsigned long long) code;
#ifdef __HIP_DEVICE_COMPILE__
    atomicMin(word, v);
#else
    if (v < *word) *word = v;
#endif
}

inline int64_t error_ordinal(unsigned long long word) { return (int64_t) (word >> 3); }
inline int error_code(unsigned long long word) { return (int) (word & 7); }

// refID and pos of record idx of the offsets `off` into the n_bytes of w, for the text; -1 / -1 when the offset lies outside
inline void error_record_host(const int64_t *off, int64_t idx, const uint8_t *w, int64_t n_bytes, int32_t &ref, int32_t &pos)
{
    const int64_t o = off[idx];
    const bool inside = o >= 0 && o + kBamPosEnd <= n_bytes;
    ref = inside ? (int32_t) le32(w + o + kBamRef) : -1;
    pos = inside ? (int32_t) le32(w + o + kBamPos) : -1;
}

// The same on device arrays, through queued copies on st.  They write P: it lives in the frame that calls dn::synced.
struct ErrorProbe {
    int64_t off = 0;
    uint8_t rec[kBamPosEnd] = {0};
};

inline int error_record_device(hipStream_t st, const int64_t *d_off, int64_t idx, const uint8_t *d_w, int64_t n_bytes, ErrorProbe &P,
                               int32_t &ref, int32_t &pos)
{
    DN_TRY(hipMemcpyAsync(&P.off, d_off + idx, sizeof(P.off), hipMemcpyDeviceToHost, st));
    DN_TRY(hipStreamSynchronize(st));
    ref = pos = -1;
    if (P.off < 0 || P.off + kBamPosEnd > n_bytes) return DN_OK;
    DN_TRY(hipMemcpyAsync(P.rec, d_w + P.off, sizeof(P.rec), hipMemcpyDeviceToHost, st));
    DN_TRY(hipStreamSynchronize(st));
    ref = (int32_t) le32(P.rec + kBamRef);
    pos = (int32_t) le32(P.rec + kBamPos);
    return DN_OK;
}

// ---- the texts that name a record -----------------------------------------------------------------------------------

inline std::string record_name(int64_t idx, int32_t ref, int32_t pos)
{
    return "record " + std::to_string(idx) + " (refID " + std::to_string(ref) + ", position " + std::to_string(pos) + ")";
}

inline int record_shape_error(const std::string &who)
{
    return fail(DN_E_INVALID, "malformed BAM " + who + ": its read name and CIGAR do not fit inside the record");
}

inline int record_reference_error(const std::string &who, int32_t n_ref)
{
    return fail(DN_E_INVALID, who + " names a reference the header does not have (" + std::to_string(n_ref) + " references)");
}

inline int record_cut_error(int64_t idx, int64_t left)
{
    return fail(DN_E_INVALID, "record " + std::to_string(idx) + " is cut by the end of the file (" + std::to_string(left) + " bytes of it are there)");
}

// what an entry point `who` of a builder handle (`noun`: "index", "sort") checks first; device: the build the entry is for
template <class H> int check_handle(H h, const char *who, const char *noun, bool device)
{
    if (!h || (h->device >= 0) != device) return fail(DN_E_INVALID, std::string(who) + ": bad argument");
    if (h->failed || h->finished) return fail(DN_E_STATE, std::string(who) + ": the " + noun + " is finished or has failed");
    return DN_OK;
}

}  // namespace dn

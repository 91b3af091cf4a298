// dn_bai.hip -- the .bai or .csi index of a coordinate-sorted BAM file, built from a pass over every record on the device.
//
// Both are one binning index (include/degnorm_amd.h): bins of 2^min_shift bases ("granules"; a .bai's 16 kb windows) in
// `depth` levels below the root.  A .bai is (14, 5) with a linear index, a .csi any (min_shift, depth) with one offset per
// bin; the builder carries the pair (Binning) and the kernels take it by value.  Below, 14 stands for min_shift.
//
// A window (the record cut by the window before + the inflated BGZF blocks of about window_bytes) is inflated
// (dn::InflateWindow) and framed (dn::frame_window, tid = -1) where it lies; then, one lane per record:
//
//   records   k_bai_records reads refID, pos, flag and the CIGAR, computes [beg, end), the bin (reg2bin), the packed
//             (refID, bin) key and the record's virtual offset -- a binary search of the window's piece table, which says for
//             every stretch of window bytes which block (file offset) and which byte of it they are; carried bytes keep the
//             pieces of the blocks they came from -- and checks order against the record before (the window's first record
//             against the carried state of the last record of the window before).  The first error wins (dn::note_error)
//   max-scan  within a reference records are sorted, so the smallest vbeg over a 16 kb window of the linear index is that
//             of the first record in file order that overlaps it.  With E(r) the largest (end - 1) >> 14 of the reference's
//             earlier records, record r claims the windows max(beg >> 14, E(r) + 1) .. (end - 1) >> 14.  refID does not
//             decrease, so E comes from one plain inclusive max-scan of refID << 32 | ((end - 1) >> 14) + 1: a later
//             reference outweighs every window of an earlier one.  No atomics and no dense per-reference array
//   flags     k_bai_flags marks run heads (the key differs from the record before) and claims (the range is not empty)
//   scatter   after two exclusive sums, k_bai_scatter writes the heads (key, vbeg, ordinal in the window, unmapped records
//             before it) and the claims (refID, first and last window, vbeg), and the last lane leaves the carried state
//
// Only these two small tables return to the host.  There they are stitched (a run that goes on across a window boundary is
// one run; a run ends where the next begins), and dn_bai_finish sorts the runs by key (stably: file order within a bin),
// joins chunks that touch in one block, and fills the linear index -- or, for a .csi, finds every bin's offset by a search
// of the claims, which are what the linear index would be filled from.
//
// The three per-record steps are __host__ __device__ functions on the record view of dn_bam_record.hpp.  The steps of a
// window are written once (run_window) over two backends: DeviceIndex queues kernels and hipcub scans on the window where it
// was inflated, HostIndex runs plain loops on bytes the caller inflated, so the index is testable without a device.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_inflate.hpp"
#include "dn_frame.hpp"
#include "dn_bam_record.hpp"

namespace {

using dn::kUnplaced;
using dn::le32;
using dn::ref_key;
using dn::reg2bin;

constexpr int kNT = 256;
constexpr int64_t kGridCap = 1 << 20;

enum { kBaiOk = 0, kBaiShape = 1, kBaiRef = 2, kBaiRefOrder = 3, kBaiPosOrder = 4, kBaiRange = 5, kBaiOffset = 6 };

// window bytes [win, the next piece's win) are the bytes uoff .. of the BGZF block at file offset coffset
struct Piece {
    int64_t win, coffset;
    int32_t uoff, pad;
};

// what the next window needs of the last record before it: any = 0 before the first record of the file
struct Carry {
    uint64_t key, emax;
    int32_t ref, pos, any, pad;
};

struct Head {
    uint64_t key, vbeg;
    int32_t idx, unmapped_before;      // the record's ordinal in its window; placed records with flag & 4 before it there
};

// the first and the last granule (of 2^min_shift bases; a .bai's 16 kb windows) of a record or of a claim
struct Span {
    uint32_t lo, hi;
};

struct Claim {
    uint64_t vbeg;
    int32_t ref;
    Span g;
    int32_t pad;
};

// The binning scheme of the builder, handed to the kernels by value: a .bai is (14, 5).  cap = 2^(min_shift + 3 depth) is the
// largest end the index can hold, so a granule index stays below 2^(3 depth) <= 2^24.
struct Binning {
    int32_t min_shift, depth;
    int64_t cap;
};
constexpr Binning kBaiBinning{14, 5, (int64_t) 1 << 29};

struct Totals {
    int64_t heads, unmapped, claims;
};

// per-record arrays of one window
struct Recs {
    uint64_t *key, *vbeg, *emax_in, *emax;       // emax: the inclusive max-scan of emax_in
    Span *win;                                   // beg >> min_shift and (end - 1) >> min_shift
    uint8_t *fl;                                 // bit 0: placed and flag & 4
    uint64_t *hs, *hs_sum;                       // head flag | unmapped flag << 32, and its exclusive sum
    int32_t *cf, *cf_sum;                        // claim flag, and its exclusive sum
};

DN_HD uint64_t piece_voffset(const Piece *pc, int32_t n_pieces, int64_t o)
{
    int32_t lo = 0, hi = n_pieces - 1;             // the last piece with win <= o; piece 0 starts at 0
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (pc[mid].win <= o) lo = mid; else hi = mid - 1;
    }
    const int64_t u = pc[lo].uoff + (o - pc[lo].win);
    return u < 65536 ? (uint64_t) pc[lo].coffset << 16 | (uint64_t) u : ~(uint64_t) 0;     // 16 bits for the place in the block
}

// Record i of the window: its entries of R, and kBaiOk or what is wrong with it.  frame_window established that the
// record lies inside the window; the bounds are checked again so that offsets that do not belong to w cannot lead outside.
DN_HD int bai_record(const uint8_t *w, int64_t n_bytes, const int64_t *rec_off, int64_t i, const Piece *pc, int32_t n_pieces,
                     int32_t n_ref, const Binning &B, const Carry &cin, const Recs &R)
{
    const int64_t o = rec_off[i];
    R.key[i] = (uint64_t) kUnplaced << 32; R.vbeg[i] = 0; R.emax_in[i] = 0; R.win[i] = Span{0, 0}; R.fl[i] = 0;
    dn::BamHead H;
    if (!dn::bam_head(w, n_bytes, o, H) || !H.names_fit()) return kBaiShape;
    const int32_t ref = H.ref, pos = H.pos;
    const uint32_t flag = H.flag;
    const int64_t n_cig = H.n_cig;
    int64_t rlen = 0;
    const uint8_t *c = w + H.cigar();
    for (int64_t k = 0; k < n_cig; k++) {
        const uint32_t op = le32(c + 4 * k), code = op & 15;
        if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) rlen += op >> 4;
    }
    if ((flag & 4) || n_cig == 0 || rlen == 0) rlen = 1;
    int64_t beg = pos, end = beg + rlen;
    if (ref >= 0) {
        if (beg < 0) beg = 0;
        if (end <= 0) end = 1;
    }
    const bool in_range = beg <= B.cap && end <= B.cap;
    const uint32_t rk = ref_key(ref);
    const uint32_t bin = ref >= 0 && in_range ? reg2bin(beg, end, B.min_shift, B.depth) : 0;
    const uint32_t bw = ref >= 0 && in_range ? (uint32_t) (beg >> B.min_shift) : 0;
    const uint32_t ew = ref >= 0 && in_range ? (uint32_t) ((end - 1) >> B.min_shift) : 0;
    R.key[i] = (uint64_t) rk << 32 | bin;
    R.vbeg[i] = piece_voffset(pc, n_pieces, o);
    // one word still holds reference and granule: pos is an int32, so even at min_shift 1 the last granule + 1 is at most
    // 2^30 (and, as end <= cap, below 2^24 + 1 in an index that accepts the record)
    R.emax_in[i] = (uint64_t) rk << 32 | (ref >= 0 ? ew + 1 : 0);
    R.win[i] = Span{bw, ew};
    R.fl[i] = ref >= 0 && (flag & 4) ? 1 : 0;
    bool has_prev = cin.any != 0;
    int32_t pref = cin.ref, ppos = cin.pos;
    if (i > 0) {
        const int64_t po = rec_off[i - 1];
        has_prev = po >= 0 && po + dn::kBamPosEnd <= n_bytes;
        if (has_prev) { pref = (int32_t) le32(w + po + dn::kBamRef); ppos = (int32_t) le32(w + po + dn::kBamPos); }
    }
    if (ref >= n_ref) return kBaiRef;
    if (has_prev && rk < ref_key(pref)) return kBaiRefOrder;
    if (has_prev && ref >= 0 && ref == pref && pos < ppos) return kBaiPosOrder;
    if (!in_range) return kBaiRange;
    if (R.vbeg[i] == ~(uint64_t) 0) return kBaiOffset;
    return kBaiOk;
}

// Is record i the head of a run, and which windows of the linear index does it claim (lo > hi: none)?
DN_HD void bai_flags(const Recs &R, int64_t i, const Carry &cin, bool &head, uint32_t &lo, uint32_t &hi)
{
    const uint64_t key = R.key[i];
    const uint64_t prev_key = i > 0 ? R.key[i - 1] : cin.any ? cin.key : ~(uint64_t) 0;
    head = key != prev_key;
    uint64_t pe = i > 0 ? R.emax[i - 1] : 0;
    if (cin.any && cin.emax > pe) pe = cin.emax;
    const uint32_t rk = (uint32_t) (key >> 32), bw = R.win[i].lo;
    const uint32_t past = (uint32_t) (pe >> 32) == rk ? (uint32_t) pe : 0;         // E + 1, or 0 for the reference's first record
    lo = bw > past ? bw : past;
    hi = R.win[i].hi;
    if (rk == kUnplaced) { lo = 1; hi = 0; }
}

DN_HD void bai_flag_pass(const Recs &R, int64_t i, const Carry &cin)
{
    bool head;
    uint32_t lo, hi;
    bai_flags(R, i, cin, head, lo, hi);
    R.hs[i] = (uint64_t) (head ? 1 : 0) | (uint64_t) (R.fl[i] & 1) << 32;
    R.cf[i] = lo <= hi ? 1 : 0;
}

DN_HD void bai_scatter_pass(const uint8_t *w, const int64_t *rec_off, const Recs &R, int64_t i, int64_t n_rec, const Carry &cin,
                            Head *heads, Claim *claims, Totals *tot, Carry *cout)
{
    bool head;
    uint32_t lo, hi;
    bai_flags(R, i, cin, head, lo, hi);
    const uint64_t s = R.hs_sum[i];
    if (head) heads[(uint32_t) s] = Head{R.key[i], R.vbeg[i], (int32_t) i, (int32_t) (s >> 32)};
    if (lo <= hi) claims[R.cf_sum[i]] = Claim{R.vbeg[i], (int32_t) (R.key[i] >> 32), Span{lo, hi}, 0};
    if (i == n_rec - 1) {
        const uint64_t t = s + R.hs[i];
        *tot = Totals{(int64_t) (uint32_t) t, (int64_t) (t >> 32), (int64_t) R.cf_sum[i] + R.cf[i]};
        const int64_t o = rec_off[i];
        uint64_t e = R.emax[i];
        if (cin.any && cin.emax > e) e = cin.emax;
        *cout = Carry{R.key[i], e, (int32_t) le32(w + o + dn::kBamRef), (int32_t) le32(w + o + dn::kBamPos), 1, 0};
    }
}

__global__ __launch_bounds__(kNT) void k_bai_records(const uint8_t *__restrict__ w, int64_t n_bytes, const int64_t *__restrict__ rec_off,
                                                     int64_t n_rec, const Piece *__restrict__ pc, int32_t n_pieces, int32_t n_ref,
                                                     Binning B, const Carry *__restrict__ cin, Recs R, unsigned long long *__restrict__ err)
{
    const Carry c = *cin;
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n_rec; i += (int64_t) gridDim.x * kNT) {
        const int e = bai_record(w, n_bytes, rec_off, i, pc, n_pieces, n_ref, B, c, R);
        if (e != kBaiOk) dn::note_error(err, i, e);
    }
}

__global__ __launch_bounds__(kNT) void k_bai_flags(int64_t n_rec, const Carry *__restrict__ cin, Recs R)
{
    const Carry c = *cin;
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n_rec; i += (int64_t) gridDim.x * kNT) bai_flag_pass(R, i, c);
}

__global__ __launch_bounds__(kNT) void k_bai_scatter(const uint8_t *__restrict__ w, const int64_t *__restrict__ rec_off, int64_t n_rec,
                                                     const Carry *__restrict__ cin, Recs R, Head *__restrict__ heads,
                                                     Claim *__restrict__ claims, Totals *__restrict__ tot, Carry *__restrict__ cout)
{
    const Carry c = *cin;
    for (int64_t i = (int64_t) blockIdx.x * kNT + threadIdx.x; i < n_rec; i += (int64_t) gridDim.x * kNT)
        bai_scatter_pass(w, rec_off, R, i, n_rec, c, heads, claims, tot, cout);
}

struct Run {
    uint64_t key, vbeg, vend;
    int64_t n, n_unmapped;
};

}  // namespace

struct dn_bai_s {
    int device = -1;                   // < 0: the host build
    int32_t n_ref = 0;
    bool csi = false;                  // a .csi builder: per-bin loffset in place of the linear index
    Binning binning = kBaiBinning;
    int64_t segment = 0;
    int64_t n_records = 0, n_windows = 0, n_fixups = 0;
    bool failed = false, finished = false;
    std::vector<Piece> carry_pieces;   // of the record cut by the end of the window before, rebased to offset 0
    std::vector<Run> runs;             // in file order
    std::vector<Claim> claims;
    // HostIndex: the bytes of the record cut by the end of the window before, and the carried state
    std::vector<uint8_t> h_carry;
    Carry h_state{0, 0, 0, 0, 0, 0};
    // DeviceIndex
    dn::Stream st;
    dn::GrowBuffer<uint8_t> win;
    dn::InflateWindow ingest;          // of dn_bai_window; armed by dn_bai_expect_crc
    dn::DeviceCarry carry;             // the bytes of the record cut by the end of the window before
    dn::GrowBuffer<int64_t> rec_off;
    dn::GrowBuffer<Piece> pieces;
    dn::GrowBuffer<uint64_t> key, vbeg, emax_in, emax, hs, hs_sum;
    dn::GrowBuffer<Span> rwin;
    dn::GrowBuffer<uint8_t> fl;
    dn::GrowBuffer<int32_t> cf, cf_sum;
    dn::GrowBuffer<Head> heads;
    dn::GrowBuffer<Claim> d_claims;
    dn::DeviceBuffer<Carry> state;     // two entries: read one, write the other
    dn::DeviceBuffer<Totals> totals;
    dn::DeviceBuffer<unsigned long long> err;
    int parity = 0;
    dn::FrameWork frame;
    dn::Scratch scratch;
    dn::Event ev2, ev3;                // around the index kernels
    // what dn_bai_finish built
    std::vector<int32_t> ref_n_bin, ref_n_intv, bin_id, bin_n_chunk;
    std::vector<uint64_t> ref_pseudo, chunks, ioffset, loffset;
    int64_t n_no_coor = 0;

    int64_t carried() const { return device < 0 ? (int64_t) h_carry.size() : carry.n; }
};

namespace {

int record_error(dn_bai h, int code, int64_t idx, int32_t ref, int32_t pos)
{
    const std::string who = dn::record_name(h->n_records + idx, ref, pos);
    switch (code) {
    case kBaiShape: return dn::record_shape_error(who);
    case kBaiRef: return dn::record_reference_error(who, h->n_ref);
    case kBaiRefOrder: return dn::fail(DN_E_INVALID, "BAM file is not sorted by coordinate: " + who + " follows a record of a later reference");
    case kBaiPosOrder: return dn::fail(DN_E_INVALID, "BAM file is not sorted by coordinate: " + who + " follows a larger position of the same reference");
    case kBaiRange:
        if (!h->csi) return dn::fail(DN_E_INVALID, who + " reaches beyond position 2^29: a .bai index cannot hold it");
        return dn::fail(DN_E_INVALID, who + " reaches beyond position 2^" + std::to_string(h->binning.min_shift + 3 * h->binning.depth) +
                                          ": a .csi index of min_shift " + std::to_string(h->binning.min_shift) + " and depth " +
                                          std::to_string(h->binning.depth) + " cannot hold it");
    default: return dn::fail(DN_E_INVALID, who + " starts beyond byte 65535 of its BGZF block: a virtual offset cannot hold it");
    }
}

// A window's pieces are those of the carried bytes, then one per block that keeps a byte.  This checks block b's file offset
// and adds its piece: `keep` bytes from byte `skip` of the block, at window offset `at`.
int add_piece(const char *who, std::vector<Piece> &pc, int64_t b, int64_t coffset, int64_t at, int32_t skip, int32_t keep)
{
    if (coffset < 0 || coffset >= ((int64_t) 1 << 48))
        return dn::fail(DN_E_INVALID, std::string(who) + ": file offset of block " + std::to_string(b) + " outside 0 .. 2^48");
    if (keep > 0) pc.push_back(Piece{at, coffset, skip, 0});
    return DN_OK;
}

// the pieces of the bytes [consumed, total) of the window, rebased: the next window's carry
void carry_pieces(dn_bai h, const std::vector<Piece> &pc, int64_t consumed, int64_t total)
{
    std::vector<Piece> out;
    for (size_t k = 0; k < pc.size(); k++) {
        const int64_t end = k + 1 < pc.size() ? pc[k + 1].win : total;
        if (end <= consumed) continue;
        const int64_t from = pc[k].win > consumed ? pc[k].win : consumed;
        out.push_back(Piece{from - consumed, pc[k].coffset, (int32_t) (pc[k].uoff + (from - pc[k].win)), 0});
    }
    h->carry_pieces.swap(out);
}

// stitch one window's tables onto the runs and claims so far
void absorb(dn_bai h, int64_t n_rec, const Totals &tot, const Head *heads, const Claim *cl)
{
    int64_t at = 0, unm = 0;
    for (int64_t j = 0; j < tot.heads; j++) {
        if (!h->runs.empty()) {
            Run &r = h->runs.back();
            r.n += heads[j].idx - at;
            r.n_unmapped += heads[j].unmapped_before - unm;
            r.vend = heads[j].vbeg;
        }
        h->runs.push_back(Run{heads[j].key, heads[j].vbeg, 0, 0, 0});
        at = heads[j].idx;
        unm = heads[j].unmapped_before;
    }
    if (!h->runs.empty()) {
        h->runs.back().n += n_rec - at;
        h->runs.back().n_unmapped += tot.unmapped - unm;
    }
    h->claims.insert(h->claims.end(), cl, cl + tot.claims);
    h->n_records += n_rec;
}

// One window on the host: plain loops over the bytes the caller inflated, behind those carried from the window before
struct HostIndex {
    dn_bai h;
    std::vector<uint8_t> win;
    std::vector<int64_t> off;
    std::vector<uint64_t> key, vbeg, emax_in, emax, hs, hs_sum;
    std::vector<Span> rwin;
    std::vector<uint8_t> fl;
    std::vector<int32_t> cf, cf_sum;
    Recs R{};
    Carry next{0, 0, 0, 0, 0, 0};
    std::vector<Head> heads;
    std::vector<Claim> cl;
    Totals tot{0, 0, 0};

    HostIndex(dn_bai h_, const uint8_t *data, int64_t n_data) : h(h_), win(h_->h_carry)
    {
        win.insert(win.end(), data, data + n_data);
        win.resize(win.size() + 16);                                    // as the device buffers: slack behind the window
    }
    int frame(int64_t total, int64_t &nr, int64_t &consumed, int64_t &fixups)
    {
        off.resize((size_t) (total / dn::kBamName + 2));
        return dn_bam_frame_segments_host(win.data(), total, -1, nullptr, h->segment, off.data(), (int64_t) off.size(), &nr, &consumed, &fixups);
    }
    // stops at the first faulty record
    int records(int64_t total, int64_t nr, const std::vector<Piece> &pc, unsigned long long &e, int32_t &ref, int32_t &pos)
    {
        const size_t n = (size_t) nr;
        key.resize(n); vbeg.resize(n); emax_in.resize(n); emax.resize(n); hs.resize(n); hs_sum.resize(n);
        rwin.resize(n); fl.resize(n); cf.resize(n); cf_sum.resize(n);
        R = Recs{key.data(), vbeg.data(), emax_in.data(), emax.data(), rwin.data(), fl.data(), hs.data(), hs_sum.data(), cf.data(), cf_sum.data()};
        for (int64_t i = 0; i < nr && e == dn::kNoError; i++) {
            const int code = bai_record(win.data(), total, off.data(), i, pc.data(), (int32_t) pc.size(), h->n_ref, h->binning, h->h_state, R);
            if (code != kBaiOk) dn::note_error(&e, i, code);
        }
        if (e != dn::kNoError) dn::error_record_host(off.data(), dn::error_ordinal(e), win.data(), total, ref, pos);
        return DN_OK;
    }
    int max_scan(int64_t nr)
    {
        for (size_t i = 0; i < (size_t) nr; i++) emax[i] = i > 0 && emax[i - 1] > emax_in[i] ? emax[i - 1] : emax_in[i];
        return DN_OK;
    }
    int flags(int64_t nr)
    {
        for (int64_t i = 0; i < nr; i++) bai_flag_pass(R, i, h->h_state);
        return DN_OK;
    }
    int sums(int64_t nr)
    {
        uint64_t s = 0;
        int32_t c = 0;
        for (size_t i = 0; i < (size_t) nr; i++) { hs_sum[i] = s; s += hs[i]; cf_sum[i] = c; c += cf[i]; }
        heads.resize((size_t) (uint32_t) s);
        cl.resize((size_t) c);
        return DN_OK;
    }
    int scatter(int64_t nr)
    {
        for (int64_t i = 0; i < nr; i++) bai_scatter_pass(win.data(), off.data(), R, i, nr, h->h_state, heads.data(), cl.data(), &tot, &next);
        return DN_OK;
    }
    int fetch(int64_t)
    {
        h->h_state = next;
        return DN_OK;
    }
    int keep(int64_t consumed, int64_t total)
    {
        h->h_carry.assign(win.begin() + consumed, win.begin() + total);
        return DN_OK;
    }
};

// The same on the device, on the window h->win and the offsets h->rec_off.  What queued copies write lives in this object,
// which dn_bai_window declares outside the body it hands to dn::synced.
struct DeviceIndex {
    dn_bai h;
    unsigned long long h_err = dn::kNoError;
    dn::ErrorProbe probe;
    Recs R{};
    const Carry *cin = nullptr;
    Carry *cout = nullptr;
    unsigned grid = 1;
    std::vector<Head> heads;
    std::vector<Claim> cl;
    Totals tot{0, 0, 0};
    double frame_ms = 0.0, index_ms = 0.0;

    int frame(int64_t total, int64_t &nr, int64_t &consumed, int64_t &fixups)
    {
        dn::FrameResult F;
        const int rc = dn::frame_window(h->st, h->frame, h->win, total, -1, nullptr, h->segment, -1, h->rec_off, F);
        nr = F.n_rec; consumed = F.consumed; fixups = F.n_fixups;
        frame_ms = F.device_ms;
        return rc;
    }
    // reports an error after the pass over the whole window
    int records(int64_t total, int64_t nr, const std::vector<Piece> &pc, unsigned long long &e, int32_t &ref, int32_t &pos)
    {
        hipStream_t st = h->st;
        DN_TRY(h->pieces.reserve((int64_t) pc.size(), 0, st));
        DN_TRY(h->key.reserve(nr, 0, st)); DN_TRY(h->vbeg.reserve(nr, 0, st)); DN_TRY(h->emax_in.reserve(nr, 0, st));
        DN_TRY(h->emax.reserve(nr, 0, st)); DN_TRY(h->hs.reserve(nr, 0, st)); DN_TRY(h->hs_sum.reserve(nr, 0, st));
        DN_TRY(h->rwin.reserve(nr, 0, st)); DN_TRY(h->fl.reserve(nr, 0, st)); DN_TRY(h->cf.reserve(nr, 0, st));
        DN_TRY(h->cf_sum.reserve(nr, 0, st)); DN_TRY(h->heads.reserve(nr, 0, st)); DN_TRY(h->d_claims.reserve(nr, 0, st));
        R = Recs{h->key.get(), h->vbeg.get(), h->emax_in.get(), h->emax.get(), h->rwin.get(), h->fl.get(), h->hs.get(), h->hs_sum.get(),
                 h->cf.get(), h->cf_sum.get()};
        cin = h->state.get() + h->parity;
        cout = h->state.get() + (h->parity ^ 1);
        grid = dn::grid_for(nr, kNT, kGridCap);
        DN_TRY(hipMemcpyAsync(h->pieces, pc.data(), sizeof(Piece) * pc.size(), hipMemcpyHostToDevice, st));
        DN_TRY(hipMemsetAsync(h->err, 0xff, sizeof(unsigned long long), st));
        DN_TRY(hipEventRecord(h->ev2, st));
        hipLaunchKernelGGL(k_bai_records, dim3(grid), dim3(kNT), 0, st, (const uint8_t *) h->win.get(), total, (const int64_t *) h->rec_off.get(), nr,
                           (const Piece *) h->pieces.get(), (int32_t) pc.size(), h->n_ref, h->binning, cin, R, h->err.get());
        DN_TRY(hipGetLastError());
        DN_TRY(hipMemcpyAsync(&h_err, h->err, sizeof(h_err), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        e = h_err;
        return e == dn::kNoError ? DN_OK : dn::error_record_device(st, h->rec_off, dn::error_ordinal(e), h->win, total, probe, ref, pos);
    }
    int max_scan(int64_t nr)
    {
        DN_TRY(h->scratch.run([&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::InclusiveScan(tmp, bytes, R.emax_in, R.emax, hipcub::Max(), (int) nr, h->st);
        }));
        return DN_OK;
    }
    int flags(int64_t nr)
    {
        hipLaunchKernelGGL(k_bai_flags, dim3(grid), dim3(kNT), 0, h->st, nr, cin, R);
        DN_TRY(hipGetLastError());
        return DN_OK;
    }
    int sums(int64_t nr)
    {
        DN_TRY(h->scratch.run([&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, R.hs, R.hs_sum, (int) nr, h->st); }));
        DN_TRY(h->scratch.run([&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, R.cf, R.cf_sum, (int) nr, h->st); }));
        return DN_OK;
    }
    int scatter(int64_t nr)
    {
        hipLaunchKernelGGL(k_bai_scatter, dim3(grid), dim3(kNT), 0, h->st, (const uint8_t *) h->win.get(), (const int64_t *) h->rec_off.get(), nr, cin, R,
                           h->heads.get(), h->d_claims.get(), h->totals.get(), cout);
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(h->ev3, h->st));
        return DN_OK;
    }
    // the two tables and their sizes come to the host; index_ms: around the index kernels
    int fetch(int64_t nr)
    {
        hipStream_t st = h->st;
        DN_TRY(hipMemcpyAsync(&tot, h->totals, sizeof(Totals), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (tot.heads < 0 || tot.heads > nr || tot.claims < 0 || tot.claims > nr) return dn::fail(DN_E_STATE, "dn_bai_window: table sizes outside the window");
        heads.resize((size_t) tot.heads);
        cl.resize((size_t) tot.claims);
        if (tot.heads > 0) DN_TRY(hipMemcpyAsync(heads.data(), h->heads, sizeof(Head) * heads.size(), hipMemcpyDeviceToHost, st));
        if (tot.claims > 0) DN_TRY(hipMemcpyAsync(cl.data(), h->d_claims, sizeof(Claim) * cl.size(), hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        h->parity ^= 1;
        float ms = 0.f;
        DN_TRY(hipEventElapsedTime(&ms, h->ev2, h->ev3));
        index_ms = ms;
        return DN_OK;
    }
    int keep(int64_t consumed, int64_t total)
    {
        DN_TRY(h->carry.keep(h->st, h->win, consumed, total));
        return DN_OK;
    }
};

// One window of `total` bytes whose pieces are pc, on either backend: frame it, run the three per-record passes with the
// scan and the two sums between them, carry the record the window end cuts, and stitch the window's tables onto the
// handle's.  Whatever fails spends the builder.
template <class B> int run_window(dn_bai h, B &be, const std::vector<Piece> &pc, int64_t total, int64_t *n_rec)
{
    const int rc = [&]() -> int {
        int64_t nr = 0, consumed = 0, fixups = 0;
        int rc = be.frame(total, nr, consumed, fixups);
        h->n_fixups += fixups;
        if (rc != DN_OK) return rc;
        if (nr > 0) {
            unsigned long long e = dn::kNoError;
            int32_t ref = -1, pos = -1;
            if ((rc = be.records(total, nr, pc, e, ref, pos)) != DN_OK) return rc;
            if (e != dn::kNoError) return record_error(h, dn::error_code(e), dn::error_ordinal(e), ref, pos);
            if ((rc = be.max_scan(nr)) != DN_OK || (rc = be.flags(nr)) != DN_OK || (rc = be.sums(nr)) != DN_OK ||
                (rc = be.scatter(nr)) != DN_OK || (rc = be.fetch(nr)) != DN_OK)
                return rc;
        }
        if ((rc = be.keep(consumed, total)) != DN_OK) return rc;
        carry_pieces(h, pc, consumed, total);
        absorb(h, nr, be.tot, be.heads.data(), be.cl.data());
        h->n_windows++;
        *n_rec = nr;
        return DN_OK;
    }();
    if (rc != DN_OK) h->failed = true;
    return rc;
}

int create_builder(const char *who, int device, int32_t n_ref, int64_t segment_bytes, bool csi, Binning binning, dn_bai *out)
{
    if (!out || n_ref < 0 || (segment_bytes != 0 && segment_bytes < dn::kFrameSegmentMin))
        return dn::fail(DN_E_INVALID, std::string(who) + ": bad argument (segment_bytes is 0 or at least 64)");
    dn_bai h = new dn_bai_s();
    h->device = device < 0 ? -1 : device;
    h->n_ref = n_ref;
    h->csi = csi;
    h->binning = binning;
    h->segment = segment_bytes;
    const int rc = [&]() -> int {
        if (device < 0) return DN_OK;
        DN_TRY(hipSetDevice(device));
        DN_TRY(h->st.create(hipStreamCreate));
        DN_TRY(dn::alloc_padded(h->state, 2));
        DN_TRY(dn::alloc_padded(h->totals, 1));
        DN_TRY(dn::alloc_padded(h->err, 1));
        DN_TRY(hipMemsetAsync(h->state, 0, 2 * sizeof(Carry), h->st));
        DN_TRY(h->ev2.create(hipEventCreate)); DN_TRY(h->ev3.create(hipEventCreate));
        DN_TRY(hipStreamSynchronize(h->st));
        return DN_OK;
    }();
    if (rc != DN_OK) { delete h; return rc; }
    *out = h;
    return DN_OK;
}

}  // namespace

extern "C" int dn_bai_create(int device, int32_t n_ref, int64_t segment_bytes, dn_bai *out)
{
    dn::clear_error();
    return create_builder("dn_bai_create", device, n_ref, segment_bytes, false, kBaiBinning, out);
}

extern "C" int dn_csi_create(int device, int32_t n_ref, int64_t segment_bytes, int32_t min_shift, int32_t depth, dn_bai *out)
{
    dn::clear_error();
    if (min_shift < 1 || min_shift > 30 || depth < 0 || depth > 8 || min_shift + 3 * depth > 54)
        return dn::fail(DN_E_INVALID, "dn_csi_create: min_shift is 1 .. 30, depth 0 .. 8 and min_shift + 3 depth at most 54");
    return create_builder("dn_csi_create", device, n_ref, segment_bytes, true,
                          Binning{min_shift, depth, (int64_t) 1 << (min_shift + 3 * depth)}, out);
}

extern "C" void dn_bai_destroy(dn_bai h)
{
    if (!h) return;
    if (h->device >= 0) {
        (void) hipSetDevice(h->device);
        if (h->st) (void) hipStreamSynchronize(h->st);
    }
    delete h;
}

extern "C" int dn_bai_expect_crc(dn_bai h, const uint32_t *crc32, int64_t n_blocks)
{
    dn::clear_error();
    if (!h) return dn::fail(DN_E_INVALID, "dn_bai_expect_crc: bad argument");
    if (h->device < 0) return dn::fail(DN_E_STATE, "dn_bai_expect_crc: a host builder is handed inflated bytes; its caller checks them");
    return h->ingest.arm("dn_bai_expect_crc", crc32, n_blocks);
}

extern "C" int dn_bai_window(dn_bai h, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                             const int32_t *isize, const int64_t *coffset, int32_t head_skip, int32_t *status, int64_t *n_rec,
                             double *inflate_ms, double *frame_ms, double *index_ms)
{
    dn::clear_error();
    if (h) h->ingest.take();
    int rc = dn::check_handle(h, "dn_bai_window", "index", true);
    if (rc != DN_OK) return rc;
    if (n_comp < 0 || (n_comp > 0 && !comp) || n_blocks < 0 || n_blocks > INT32_MAX ||
        (n_blocks > 0 && (!pay_off || !pay_len || !isize || !coffset || !status)) || head_skip < 0 || !n_rec)
        return dn::fail(DN_E_INVALID, "dn_bai_window: bad argument");
    std::vector<Piece> pc(h->carry_pieces);
    int64_t total = 0;
    rc = h->ingest.plan("dn_bai_window", "dn_bai_expect_crc", n_comp, n_blocks, pay_off, pay_len, isize, head_skip, -1, h->carry.n, total);
    for (int64_t b = 0; b < n_blocks && rc == DN_OK; b++) {
        const dn::InflateBlock &B = h->ingest.blk[(size_t) b];
        rc = add_piece("dn_bai_window", pc, b, coffset[b], B.dst_off, B.skip, B.keep);
    }
    if (rc != DN_OK) return rc;
    if (total > INT32_MAX) return dn::window_size_error("dn_bai_window");
    hipStream_t st = h->st;
    DN_TRY(hipSetDevice(h->device));
    *n_rec = 0;
    if (inflate_ms) *inflate_ms = 0.0;
    DeviceIndex be{h};
    rc = dn::synced(st, [&]() -> int {
        DN_TRY(h->win.reserve(total, 0, st));
        DN_TRY(h->carry.put(st, h->win));                   // the record cut by the end of the window before goes first
        bool ok = true;
        const int wrc = h->ingest.run(st, comp, n_comp, h->win, status, inflate_ms, ok);
        if (wrc != DN_OK) return wrc;
        if (!ok) { h->failed = true; return DN_OK; }        // the caller reads the statuses
        return run_window(h, be, pc, total, n_rec);
    });
    if (frame_ms) *frame_ms = be.frame_ms;
    if (index_ms) *index_ms = be.index_ms;
    return rc;
}

extern "C" int dn_bai_window_host(dn_bai h, const uint8_t *data, int64_t n_data, int64_t n_blocks, const int32_t *isize, const int64_t *coffset,
                                  int32_t head_skip, int64_t *n_rec)
{
    dn::clear_error();
    int rc = dn::check_handle(h, "dn_bai_window_host", "index", false);
    if (rc != DN_OK) return rc;
    if (n_data < 0 || (n_data > 0 && !data) || n_blocks < 0 || (n_blocks > 0 && (!isize || !coffset)) || head_skip < 0 || !n_rec)
        return dn::fail(DN_E_INVALID, "dn_bai_window_host: bad argument");
    std::vector<Piece> pc(h->carry_pieces);
    int64_t total = h->carried(), sum = 0, skip = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
        if (isize[b] < 0) return dn::fail(DN_E_INVALID, "dn_bai_window_host: block " + std::to_string(b) + " has a negative inflated size");
        int32_t lo, keep;
        dn::window_trim(b, n_blocks, isize[b], head_skip, -1, lo, keep);
        if ((rc = add_piece("dn_bai_window_host", pc, b, coffset[b], total, lo, keep)) != DN_OK) return rc;
        if (b == 0) skip = lo;
        total += keep;
        sum += isize[b];
    }
    if (total > INT32_MAX) return dn::window_size_error("dn_bai_window_host");
    if (sum != n_data) return dn::fail(DN_E_INVALID, "dn_bai_window_host: the blocks' sizes do not add up to n_data");
    HostIndex be(h, data + skip, n_data - skip);
    return run_window(h, be, pc, total, n_rec);
}

extern "C" int dn_bai_finish(dn_bai h, int64_t end_voffset, int64_t *sizes)
{
    dn::clear_error();
    if (!h || !sizes || end_voffset < 0) return dn::fail(DN_E_INVALID, "dn_bai_finish: bad argument");
    if (h->failed || h->finished) return dn::fail(DN_E_STATE, "dn_bai_finish: the index is finished or has failed");
    if (h->carried() > 0) {
        h->failed = true;
        return dn::record_cut_error(h->n_records, h->carried());
    }
    const size_t n_ref = (size_t) h->n_ref;
    if (!h->runs.empty()) h->runs.back().vend = (uint64_t) end_voffset;
    h->ref_n_bin.assign(n_ref, 0);
    h->ref_n_intv.assign(n_ref, 0);
    h->ref_pseudo.assign(4 * n_ref, 0);
    std::vector<uint8_t> seen(n_ref, 0);
    std::vector<size_t> order;
    for (size_t k = 0; k < h->runs.size(); k++) {
        const Run &r = h->runs[k];
        const uint32_t ref = (uint32_t) (r.key >> 32);
        if (ref == kUnplaced) { h->n_no_coor += r.n; continue; }
        uint64_t *p = &h->ref_pseudo[4 * (size_t) ref];
        if (!seen[ref]) { seen[ref] = 1; p[0] = r.vbeg; }
        p[1] = r.vend;
        p[2] += (uint64_t) (r.n - r.n_unmapped);
        p[3] += (uint64_t) r.n_unmapped;
        order.push_back(k);
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return h->runs[a].key < h->runs[b].key; });
    // chunks of a bin in file order; one that begins in the block the one before it ends in is joined to it
    uint64_t cur = ~(uint64_t) 0;
    for (size_t k : order) {
        const Run &r = h->runs[k];
        if (r.key != cur) {
            cur = r.key;
            h->bin_id.push_back((int32_t) (uint32_t) r.key);
            h->bin_n_chunk.push_back(0);
            h->ref_n_bin[(size_t) (r.key >> 32)]++;
        } else if (h->chunks.back() >> 16 >= r.vbeg >> 16) {
            h->chunks.back() = r.vend;
            continue;
        }
        h->chunks.push_back(r.vbeg);
        h->chunks.push_back(r.vend);
        h->bin_n_chunk.back()++;
    }
    // the linear index: claims are in file order, so per reference ascending and disjoint; a window nobody claimed takes
    // the value of the next one that was
    std::vector<int64_t> ioff_at(n_ref + 1, 0);
    if (h->csi) {
        // no dense table: the back-filled linear index at a bin's first granule is the vbeg of the reference's first claim whose
        // last granule is at or beyond it -- one exists, since a record of the bin ends beyond the bin's start
        std::vector<size_t> claim_at(n_ref + 1, 0);
        for (const Claim &c : h->claims) claim_at[(size_t) c.ref + 1]++;
        for (size_t r = 0; r < n_ref; r++) claim_at[r + 1] += claim_at[r];
        const int depth = h->binning.depth;
        size_t b = 0;
        for (size_t r = 0; r < n_ref; r++)
            for (int32_t k = 0; k < h->ref_n_bin[r]; k++, b++) {
                const uint32_t bin = (uint32_t) h->bin_id[b];
                int level = 0;
                uint32_t first = 0;                                     // the first bin of the level
                while (level < depth && bin >= first + ((uint32_t) 1 << 3 * level)) { first += (uint32_t) 1 << 3 * level; level++; }
                const uint32_t g0 = (bin - first) << 3 * (depth - level);
                const Claim *lo = h->claims.data() + claim_at[r], *hi = h->claims.data() + claim_at[r + 1];
                const Claim *at = std::partition_point(lo, hi, [&](const Claim &c) { return c.g.hi < g0; });
                h->loffset.push_back(at != hi ? at->vbeg : 0);
            }
    } else {
        for (const Claim &c : h->claims) {
            const int32_t hi = (int32_t) c.g.hi + 1;
            if (hi > h->ref_n_intv[(size_t) c.ref]) h->ref_n_intv[(size_t) c.ref] = hi;
        }
        for (size_t r = 0; r < n_ref; r++) ioff_at[r + 1] = ioff_at[r] + h->ref_n_intv[r];
        h->ioffset.assign((size_t) ioff_at[n_ref], ~(uint64_t) 0);
        for (const Claim &c : h->claims)
            for (uint32_t wdw = c.g.lo; wdw <= c.g.hi; wdw++) h->ioffset[(size_t) (ioff_at[(size_t) c.ref] + wdw)] = c.vbeg;
        for (size_t r = 0; r < n_ref; r++)
            for (int64_t wdw = ioff_at[r + 1] - 2; wdw >= ioff_at[r]; wdw--)
                if (h->ioffset[(size_t) wdw] == ~(uint64_t) 0) h->ioffset[(size_t) wdw] = h->ioffset[(size_t) wdw + 1];
    }
    h->finished = true;
    sizes[0] = (int64_t) h->bin_id.size();
    sizes[1] = (int64_t) h->chunks.size() / 2;
    sizes[2] = (int64_t) h->ioffset.size();
    sizes[3] = h->n_records;
    sizes[4] = h->n_no_coor;
    sizes[5] = h->n_windows;
    sizes[6] = h->n_fixups;
    return DN_OK;
}

extern "C" int dn_bai_fetch(dn_bai h, int32_t *ref_n_bin, int32_t *ref_n_intv, uint64_t *ref_pseudo, int32_t *bin_id, int32_t *bin_n_chunk,
                            uint64_t *chunks, uint64_t *ioffset)
{
    dn::clear_error();
    if (!h || !ref_n_bin || !ref_n_intv || !ref_pseudo || !bin_id || !bin_n_chunk || !chunks || (!ioffset && !h->csi))
        return dn::fail(DN_E_INVALID, "dn_bai_fetch: bad argument");
    if (!h->finished) return dn::fail(DN_E_STATE, "dn_bai_fetch: dn_bai_finish first");
    std::copy(h->ref_n_bin.begin(), h->ref_n_bin.end(), ref_n_bin);
    std::copy(h->ref_n_intv.begin(), h->ref_n_intv.end(), ref_n_intv);
    std::copy(h->ref_pseudo.begin(), h->ref_pseudo.end(), ref_pseudo);
    std::copy(h->bin_id.begin(), h->bin_id.end(), bin_id);
    std::copy(h->bin_n_chunk.begin(), h->bin_n_chunk.end(), bin_n_chunk);
    std::copy(h->chunks.begin(), h->chunks.end(), chunks);
    std::copy(h->ioffset.begin(), h->ioffset.end(), ioffset);
    return DN_OK;
}

extern "C" int dn_csi_loffset(dn_bai h, uint64_t *loffset)
{
    dn::clear_error();
    if (!h || !loffset) return dn::fail(DN_E_INVALID, "dn_csi_loffset: bad argument");
    if (!h->csi) return dn::fail(DN_E_STATE, "dn_csi_loffset: a .bai builder has a linear index, no per-bin offsets");
    if (!h->finished) return dn::fail(DN_E_STATE, "dn_csi_loffset: dn_bai_finish first");
    std::copy(h->loffset.begin(), h->loffset.end(), loffset);
    return DN_OK;
}

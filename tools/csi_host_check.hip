// csi_host_check.hip -- the host build of the index builder (csrc/dn_bai.hip: dn_bai_create / dn_csi_create, dn_bai_window_host,
// dn_bai_finish, dn_bai_fetch, dn_csi_loffset) under the host sanitizers, as a program of its own: nothing is loaded into
// Python and no device is touched.  Seeded streams of sorted records (short reads, spliced reads across every level's
// boundaries, flag 4, no CIGAR, unplaced tails) go through the builder at several (min_shift, depth) and as a .bai, window
// by window, from buffers of exactly their size -- a read past the last record is a read past the buffer -- and the
// tables that come back are held to a record-by-record restatement: the set of bins of every reference, every bin's
// loffset (the first record whose end lies beyond the bin's start), the .bai's linear index, the pseudo-bins' counts and
// n_no_coor.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/csi_host_check.hip degnorm_amd/csrc/dn_bai.hip degnorm_amd/csrc/dn_frame.hip degnorm_amd/csrc/dn_inflate.hip \
//         -o csi_host_check && ./csi_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the three functions below, so the units link alone.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

struct Rec {
    int32_t ref, pos;
    uint32_t flag;
    std::vector<uint32_t> cigar;                     // len << 4 | op; M = 0, N = 3
    int64_t beg, end, at;                            // as the index sees it; its first byte in the stream
};

static uint64_t g_seed;
static uint32_t rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (g_seed >> 33); }

static void put32(std::vector<uint8_t> &out, uint32_t v) { for (int k = 0; k < 4; k++) out.push_back((uint8_t) (v >> 8 * k)); }

static void encode(std::vector<uint8_t> &out, Rec &r, int k)
{
    char name[16];
    const int l_name = snprintf(name, sizeof name, "r%d", k % 1000) + 1;
    r.at = (int64_t) out.size();
    put32(out, (uint32_t) (32 + l_name + 4 * r.cigar.size()));
    put32(out, (uint32_t) r.ref); put32(out, (uint32_t) r.pos);
    put32(out, (uint32_t) l_name | 60u << 8 | 4680u << 16);
    put32(out, (uint32_t) r.cigar.size() | r.flag << 16);
    put32(out, 0); put32(out, 0xffffffffu); put32(out, 0xffffffffu); put32(out, 0);
    out.insert(out.end(), name, name + l_name);
    for (uint32_t op : r.cigar) put32(out, op);
    int64_t rlen = 0;
    for (uint32_t op : r.cigar) if ((op & 15) == 0 || (op & 15) == 3) rlen += op >> 4;
    if ((r.flag & 4) || r.cigar.empty() || rlen == 0) rlen = 1;
    r.beg = r.pos; r.end = r.beg + rlen;
    if (r.ref >= 0) { if (r.beg < 0) r.beg = 0; if (r.end <= 0) r.end = 1; }
}

static uint32_t spec_bin(int64_t beg, int64_t end, int min_shift, int depth)
{
    int l = depth, s = min_shift;
    int64_t t = (((int64_t) 1 << 3 * depth) - 1) / 7;
    --end;
    while (l > 0) {
        if (beg >> s == end >> s) return (uint32_t) (t + (beg >> s));
        --l; s += 3; t -= (int64_t) 1 << 3 * l;
    }
    return 0;
}

static int64_t bin_start(uint32_t bin, int min_shift, int depth)
{
    int l = 0;
    int64_t t = 0;
    while (l < depth && bin >= t + ((int64_t) 1 << 3 * l)) { t += (int64_t) 1 << 3 * l; l++; }
    return (int64_t) (bin - t) << (min_shift + 3 * (depth - l));
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s: ", name); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_error.c_str()); return 1; } } while (0)

// the references' lengths: `span` bases each; csi: dn_csi_create(min_shift, depth), else dn_bai_create
static int check(const char *name, uint64_t seed, int n_ref, int64_t span, int n_per_ref, bool csi, int min_shift, int depth, int blocks_per_window)
{
    g_seed = seed;
    std::vector<Rec> recs;
    const int64_t cap = (int64_t) 1 << (min_shift + 3 * depth);
    for (int ref = 0; ref < n_ref; ref++) {
        if (ref == 1 && n_ref > 2) continue;                                             // a reference without records
        std::vector<Rec> part;
        for (int k = 0; k < n_per_ref; k++) {
            Rec r{ref, (int32_t) (rnd() % (uint64_t) std::min<int64_t>(span, cap)), 0, {}, 0, 0, 0};
            const uint32_t kind = rnd() % 8;
            int64_t len = kind < 4 ? 50 : kind == 4 ? 1 : kind == 5 ? (int64_t) 1 << (min_shift + 3 * (rnd() % (depth + 1))) : 1 + rnd() % 5000;
            if (kind == 6) r.flag = 4;
            if (kind == 7 && k % 3 == 0) len = cap;                                    // some reach the cap exactly
            len = std::min<int64_t>(std::min<int64_t>(len, cap - r.pos), ((int64_t) 1 << 28) - 1);
            if (kind != 6 && !(kind == 4 && k % 2)) {                                    // kind 4, odd k: no CIGAR
                if (len <= 2) r.cigar = {(uint32_t) len << 4};
                else r.cigar = {1u << 4, (uint32_t) (len - 2) << 4 | 3u, 1u << 4};
            }
            part.push_back(r);
        }
        std::stable_sort(part.begin(), part.end(), [](const Rec &a, const Rec &b) { return a.pos < b.pos; });
        recs.insert(recs.end(), part.begin(), part.end());
    }
    int64_t n_unplaced = 17;
    for (int k = 0; k < n_unplaced; k++) recs.push_back(Rec{-1, -1, 4, {}, 0, 0, 0});
    std::vector<uint8_t> stream;
    for (size_t k = 0; k < recs.size(); k++) encode(stream, recs[k], (int) k);
    // blocks of seeded sizes; block b lies at file offset 70000 b
    std::vector<int64_t> block_at{0};
    while (block_at.back() < (int64_t) stream.size()) block_at.push_back(std::min<int64_t>((int64_t) stream.size(), block_at.back() + 1 + rnd() % 0xff00));
    const int64_t n_blocks = (int64_t) block_at.size() - 1;
    const auto voffset = [&](int64_t u) {
        const int64_t b = (int64_t) (std::upper_bound(block_at.begin(), block_at.end(), u) - block_at.begin()) - 1;
        return b >= n_blocks ? (uint64_t) (70000 * n_blocks) << 16 : (uint64_t) (70000 * b) << 16 | (uint64_t) (u - block_at[(size_t) b]);
    };
    dn_bai h = nullptr;
    int rc = csi ? dn_csi_create(-1, n_ref, 0, min_shift, depth, &h) : dn_bai_create(-1, n_ref, 0, &h);
    CHECK(rc == DN_OK, "create rc %d", rc);
    int64_t total_rec = 0;
    for (int64_t b = 0; b < n_blocks; b += blocks_per_window) {
        const int64_t e = std::min(n_blocks, b + blocks_per_window);
        const std::vector<uint8_t> data(stream.begin() + block_at[(size_t) b], stream.begin() + block_at[(size_t) e]);    // exactly the window
        std::vector<int32_t> isize;
        std::vector<int64_t> coffset;
        for (int64_t k = b; k < e; k++) { isize.push_back((int32_t) (block_at[(size_t) k + 1] - block_at[(size_t) k])); coffset.push_back(70000 * k); }
        int64_t n_rec = 0;
        rc = dn_bai_window_host(h, data.data(), (int64_t) data.size(), e - b, isize.data(), coffset.data(), 0, &n_rec);
        CHECK(rc == DN_OK, "window at block %lld rc %d", (long long) b, rc);
        total_rec += n_rec;
    }
    int64_t sizes[8] = {0};
    rc = dn_bai_finish(h, (int64_t) (70000 * n_blocks) << 16, sizes);
    CHECK(rc == DN_OK, "finish rc %d", rc);
    CHECK(total_rec == (int64_t) recs.size() && sizes[3] == total_rec && sizes[4] == n_unplaced, "%lld records, %lld without a reference", (long long) sizes[3], (long long) sizes[4]);
    CHECK(csi ? sizes[2] == 0 : sizes[2] > 0, "%lld linear-index entries", (long long) sizes[2]);
    // vectors of exactly the sizes dn_bai_finish gave
    std::vector<int32_t> ref_n_bin((size_t) n_ref), ref_n_intv((size_t) n_ref), bin_id((size_t) sizes[0]), bin_n_chunk((size_t) sizes[0]);
    std::vector<uint64_t> pseudo(4 * (size_t) n_ref), chunks(2 * (size_t) sizes[1]), ioffset((size_t) sizes[2]), loffset((size_t) sizes[0]);
    rc = dn_bai_fetch(h, ref_n_bin.data(), ref_n_intv.data(), pseudo.data(), bin_id.data(), bin_n_chunk.data(), chunks.data(), ioffset.data());
    CHECK(rc == DN_OK, "fetch rc %d", rc);
    rc = dn_csi_loffset(h, loffset.data());
    CHECK(csi ? rc == DN_OK : rc == DN_E_STATE, "loffset rc %d", rc);
    dn_bai_destroy(h);
    size_t b = 0, w = 0, c = 0;
    for (int ref = 0; ref < n_ref; ref++) {
        std::map<uint32_t, int> want;
        std::vector<const Rec *> mine;
        for (const Rec &r : recs) if (r.ref == ref) { want[spec_bin(r.beg, r.end, min_shift, depth)]++; mine.push_back(&r); }
        CHECK((size_t) ref_n_bin[(size_t) ref] == want.size(), "reference %d: %d bins, expected %zu", ref, ref_n_bin[(size_t) ref], want.size());
        CHECK(pseudo[4 * (size_t) ref + 2] + pseudo[4 * (size_t) ref + 3] == mine.size(), "reference %d: pseudo-bin counts", ref);
        auto it = want.begin();
        for (int32_t k = 0; k < ref_n_bin[(size_t) ref]; k++, b++, ++it) {
            CHECK((uint32_t) bin_id[b] == it->first, "reference %d: bin %d, expected %u", ref, bin_id[b], it->first);
            CHECK(bin_n_chunk[b] >= 1 && bin_n_chunk[b] <= it->second, "reference %d bin %d: %d chunks of %d records", ref, bin_id[b], bin_n_chunk[b], it->second);
            for (int32_t j = 0; j < bin_n_chunk[b]; j++, c++) CHECK(chunks[2 * c] < chunks[2 * c + 1], "reference %d bin %d: empty chunk", ref, bin_id[b]);
            if (!csi) continue;
            const int64_t start = bin_start(it->first, min_shift, depth);
            uint64_t expect = 0;
            for (const Rec *r : mine) if (r->end > start) { expect = voffset(r->at); break; }
            CHECK(loffset[b] == expect, "reference %d bin %d: loffset %llx, expected %llx", ref, bin_id[b], (unsigned long long) loffset[b], (unsigned long long) expect);
        }
        if (!csi) {
            int64_t n_intv = 0;
            for (const Rec *r : mine) n_intv = std::max(n_intv, ((r->end - 1) >> 14) + 1);
            CHECK(ref_n_intv[(size_t) ref] == n_intv, "reference %d: %d linear-index entries, expected %lld", ref, ref_n_intv[(size_t) ref], (long long) n_intv);
            for (int64_t g = 0; g < n_intv; g++, w++) {
                uint64_t expect = 0;
                for (const Rec *r : mine) if (r->end > g << 14) { expect = voffset(r->at); break; }
                CHECK(ioffset[w] == expect, "reference %d window %lld: %llx, expected %llx", ref, (long long) g, (unsigned long long) ioffset[w], (unsigned long long) expect);
            }
        } else
            CHECK(ref_n_intv[(size_t) ref] == 0, "reference %d: a .csi builder with a linear index", ref);
    }
    CHECK(b == (size_t) sizes[0] && c == (size_t) sizes[1] && w == (size_t) sizes[2], "tables not used up");
    printf("%-14s %6zu records, %5lld bins, %5lld chunks, %3lld blocks: ok\n", name, recs.size(), (long long) sizes[0], (long long) sizes[1], (long long) n_blocks);
    return 0;
}

int main()
{
    int bad = 0;
    bad += check("bai", 1, 3, 3000000, 3000, false, 14, 5, 1000);
    bad += check("bai_windows", 2, 3, 3000000, 3000, false, 14, 5, 1);
    bad += check("csi_14_5", 3, 3, 3000000, 3000, true, 14, 5, 2);
    bad += check("csi_4_3", 4, 2, 8192, 2500, true, 4, 3, 1);
    bad += check("csi_4_6", 5, 3, ((int64_t) 1 << 21) + 5000, 2500, true, 4, 6, 3);
    bad += check("csi_14_6", 6, 2, ((int64_t) 1 << 29) + 65536, 2500, true, 14, 6, 1000);
    bad += check("csi_1_8", 7, 2, (int64_t) 1 << 25, 2000, true, 1, 8, 2);
    bad += check("csi_30_0", 8, 2, (int64_t) 1 << 30, 1000, true, 30, 0, 1);
    bad += check("csi_one", 9, 1, 100000, 1, true, 14, 2, 1);
    // what the builder refuses: parameters out of range, and a record one base beyond the cap
    dn_bai h = nullptr;
    if (dn_csi_create(-1, 1, 0, 0, 5, &h) == DN_OK || dn_csi_create(-1, 1, 0, 31, 0, &h) == DN_OK || dn_csi_create(-1, 1, 0, 14, 9, &h) == DN_OK ||
        dn_csi_create(-1, 1, 0, 14, -1, &h) == DN_OK) { fprintf(stderr, "parameters out of range accepted\n"); bad++; }
    {
        Rec r{0, 8192 - 10, 0, {11u << 4}, 0, 0, 0};
        std::vector<uint8_t> one;
        encode(one, r, 0);
        const int32_t isize = (int32_t) one.size();
        const int64_t coffset = 0;
        int64_t n_rec = 0;
        if (dn_csi_create(-1, 1, 0, 4, 3, &h) != DN_OK || dn_bai_window_host(h, one.data(), isize, 1, &isize, &coffset, 0, &n_rec) != DN_E_INVALID ||
            g_error != "record 0 (refID 0, position 8182) reaches beyond position 2^13: a .csi index of min_shift 4 and depth 3 cannot hold it") {
            fprintf(stderr, "range error: %s\n", g_error.c_str());
            bad++;
        }
        dn_bai_destroy(h);
    }
    return bad ? 1 : 0;
}

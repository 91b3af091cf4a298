// mate_host_check.hip -- dn_bam_mate_host (csrc/dn_pair.hip) under the host sanitizers, as a program of its own: nothing is
// loaded into Python and no device is touched.  Rows of tests/test_mate_host.py (0 .. 3 rows, names that are prefixes of each
// other, one name at several loci, pos_first == pos_last, next_pos = -1, a seeded set) go through the host entry and are held
// against std::stable_sort on (padded name, (uint32) (pos_first + 1), (uint32) (pos_last + 1)).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/mate_host_check.hip degnorm_amd/csrc/dn_pair.hip -o mate_host_check && ./mate_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the three functions below, so the unit links alone.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

struct Row {
    std::string name;
    int64_t pos;
    int32_t next_pos;
    uint16_t flag;
};

static int check(const char *what, const std::vector<Row> &rows)
{
    const int64_t n = (int64_t) rows.size();
    // exactly the bytes of the names and one element per row, no slack: a read past the end is a read past the buffer
    std::vector<uint8_t> names;
    std::vector<int64_t> beg, pos;
    std::vector<int32_t> len, next_pos;
    std::vector<uint16_t> flag;
    size_t width = 0;
    for (const Row &r : rows) {
        beg.push_back((int64_t) names.size());
        len.push_back((int32_t) r.name.size());
        names.insert(names.end(), r.name.begin(), r.name.end());
        pos.push_back(r.pos); next_pos.push_back(r.next_pos); flag.push_back(r.flag);
        width = std::max(width, r.name.size());
    }
    std::vector<int32_t> order((size_t) n), pair_id((size_t) n);
    int64_t n_ids = -1;
    const int rc = dn_bam_mate_host(n, beg.data(), len.data(), names.data(), pos.data(), next_pos.data(), flag.data(), order.data(), pair_id.data(), &n_ids);
    if (rc != DN_OK) { fprintf(stderr, "%s: rc %d (%s)\n", what, rc, g_error.c_str()); return 1; }
    typedef std::tuple<std::string, uint32_t, uint32_t> Key;    // std::string compares as unsigned bytes
    std::vector<Key> key;
    for (const Row &r : rows) {
        const uint32_t p = (uint32_t) r.pos + 1u, q = (uint32_t) r.next_pos + 1u;
        const bool first = (r.flag & 0x40) != 0;
        key.emplace_back(r.name + std::string(width - r.name.size(), '\0'), first ? p : q, first ? q : p);
    }
    std::vector<int32_t> expect((size_t) n);
    std::iota(expect.begin(), expect.end(), 0);
    std::stable_sort(expect.begin(), expect.end(), [&](int32_t a, int32_t b) { return key[(size_t) a] < key[(size_t) b]; });
    int32_t id = 0;
    for (int64_t i = 0; i < n; i++) {
        if (i > 0 && key[(size_t) expect[(size_t) i]] != key[(size_t) expect[(size_t) i - 1]]) id++;
        if (order[(size_t) i] != expect[(size_t) i] || pair_id[(size_t) i] != id) {
            fprintf(stderr, "%s: position %lld: row %d id %d, expected row %d id %d\n", what, (long long) i, order[(size_t) i], pair_id[(size_t) i],
                    expect[(size_t) i], id);
            return 1;
        }
    }
    if (n_ids != (n ? id + 1 : 0)) { fprintf(stderr, "%s: %lld ids, expected %d\n", what, (long long) n_ids, n ? id + 1 : 0); return 1; }
    printf("%-12s %6lld rows, %6lld ids: ok\n", what, (long long) n, (long long) n_ids);
    return 0;
}

int main()
{
    int bad = 0;
    bad += check("empty", {});
    bad += check("one", {{"b", 5, 9, 0x43}});
    bad += check("two", {{"b", 5, 9, 0x43}, {"b", 9, 5, 0x83}});
    bad += check("three", {{"b", 9, 5, 0x83}, {"a", 1, 2, 0x41}, {"b", 5, 9, 0x41}});
    bad += check("prefix", {{"r10", 1, 2, 0x41}, {"r1", 1, 2, 0x41}, {"r1.a", 2, 1, 0x81}, {"r", 7, 7, 0x41}, {"r1", 2, 1, 0x81}, {"", 3, 4, 0x41},
                            {"r10", 2, 1, 0x81}, {"", 4, 3, 0x81}});
    bad += check("two_loci", {{"t", 100, 300, 0x41}, {"t", 5000, 5200, 0x41}, {"t", 300, 100, 0x81}, {"t", 5200, 5000, 0x81}, {"t", 100, 301, 0x41}});
    bad += check("same_pos", {{"s", 40, 40, 0x41}, {"s", 40, 40, 0x81}, {"s", 40, 41, 0x81}, {"s", 41, 40, 0x41}});
    bad += check("no_mate_pos", {{"u", 7, -1, 0x41}, {"u", 7, -1, 0x81}, {"u", 0, -1, 0x81}, {"u", -1, -1, 0x41}, {"u", 2147483647, -1, 0x41}});
    bad += check("ninth_byte", {{"abcdefghz", 3, 4, 0x41}, {"abcdefgh", 3, 4, 0x41}, {"abcdefghz", 4, 3, 0x81}, {"abcdefgh", 4, 3, 0x81}});
    uint64_t s = 2468;                                // a fixed linear congruential sequence
    const auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); };
    std::vector<Row> rows;
    for (int i = 0; i < 20000; i++) {
        std::string k(next() % 2 ? 9 + next() % 3 : next() % 4, 'p');      // around the 8-byte chunk, and short ones
        for (size_t c = k.size() > 2 ? k.size() - 2 : 0; c < k.size(); c++) k[c] = (char) ('a' + next() % 3);
        const int64_t p = next() % 8, q = (int64_t) (next() % 9) - 1;
        const bool first = next() % 2;
        rows.push_back(Row{k, first ? p : q < 0 ? 0 : q, (int32_t) (first ? q : p), (uint16_t) (first ? 0x41 : 0x81)});
    }
    bad += check("random", rows);
    return bad ? 1 : 0;
}

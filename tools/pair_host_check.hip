// pair_host_check.hip -- dn_bam_pair_host (csrc/dn_pair.hip) under the host sanitizers, as a program of its own: nothing is
// loaded into Python and no device is touched.  Key sets of tests/test_pair_host.py (chunk boundaries, prefixes, the empty
// key, bytes >= 0x80, a random set) go through the host entry and are held against std::stable_sort on the padded keys.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/pair_host_check.hip degnorm_amd/csrc/dn_pair.hip -o pair_host_check && ./pair_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the three functions below, so the unit links alone.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

static int check(const char *name, const std::vector<std::string> &keys)
{
    const int64_t n = (int64_t) keys.size();
    // exactly the bytes of the keys, no slack: a read past a key's end is a read past the buffer for the last key
    std::vector<uint8_t> names;
    std::vector<int64_t> beg;
    std::vector<int32_t> len;
    size_t width = 0;
    for (const std::string &k : keys) {
        beg.push_back((int64_t) names.size());
        len.push_back((int32_t) k.size());
        names.insert(names.end(), k.begin(), k.end());
        width = std::max(width, k.size());
    }
    std::vector<int32_t> order((size_t) n), pair_id((size_t) n);
    int64_t n_ids = -1;
    const int rc = dn_bam_pair_host(n, beg.data(), len.data(), names.data(), order.data(), pair_id.data(), &n_ids);
    if (rc != DN_OK) { fprintf(stderr, "%s: rc %d (%s)\n", name, rc, g_error.c_str()); return 1; }
    std::vector<std::string> padded;
    for (const std::string &k : keys) padded.push_back(k + std::string(width - k.size(), '\0'));
    std::vector<int32_t> expect((size_t) n);
    std::iota(expect.begin(), expect.end(), 0);
    std::stable_sort(expect.begin(), expect.end(), [&](int32_t a, int32_t b) { return padded[(size_t) a] < padded[(size_t) b]; });   // std::string compares as unsigned bytes
    int32_t id = 0;
    for (int64_t i = 0; i < n; i++) {
        if (i > 0 && padded[(size_t) expect[(size_t) i]] != padded[(size_t) expect[(size_t) i - 1]]) id++;
        if (order[(size_t) i] != expect[(size_t) i] || pair_id[(size_t) i] != id) {
            fprintf(stderr, "%s: position %lld: row %d id %d, expected row %d id %d\n", name, (long long) i, order[(size_t) i], pair_id[(size_t) i],
                    expect[(size_t) i], id);
            return 1;
        }
    }
    if (n_ids != (n ? id + 1 : 0)) { fprintf(stderr, "%s: %lld ids, expected %d\n", name, (long long) n_ids, n ? id + 1 : 0); return 1; }
    printf("%-12s %6lld keys, %6lld ids: ok\n", name, (long long) n, (long long) n_ids);
    return 0;
}

int main()
{
    int bad = 0;
    bad += check("empty", {});
    bad += check("one", {"b"});
    bad += check("three", {"b", "a", "b"});
    bad += check("prefix", {"r10", "r1.a", "r1", "r1.a", "r10", "r1", "r", "", "r1.a.b", ""});
    bad += check("ninth_byte", {"abcdefghz", "abcdefgha", "abcdefgh", "abcdefghm", "abcdefgha", "abcdefghzz", "abcdefghz"});
    bad += check("first_byte", {"q-tail-of-11", "b-tail-of-11", "z-tail-of-11", "b-tail-of-11", "a-tail-of-11"});
    bad += check("high_bytes", {"\x80" "a", "\x7f" "z", "\xff", "\x80", "a\xfe", "a\x7f", "\xff\x01", "\x80" "a", "abcdefgh\xc3\xa9", "abcdefgh\x7f"});
    bad += check("all_equal", std::vector<std::string>(9, "same.key"));
    for (int width : {1, 7, 8, 9, 16, 17, 40}) {
        std::vector<std::string> keys;
        for (int i = 0; i < 60; i++) {
            std::string k((size_t) width, 'p');
            k[(size_t) width - 1] = (char) ('a' + i * 7 % 3);
            if (width > 1) k[(size_t) width - 2] = (char) ('a' + i * 5 % 3);
            keys.push_back(k);
        }
        bad += check(("width" + std::to_string(width)).c_str(), keys);
    }
    uint64_t s = 12345;                               // a fixed linear congruential sequence
    const auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); };
    std::vector<std::string> pool, keys;
    for (int i = 0; i < 7000; i++) {
        std::string k(next() % 41, '\0');
        for (char &c : k) c = (char) (1 + next() % 255);
        pool.push_back(k);
    }
    for (int i = 0; i < 20000; i++) keys.push_back(pool[next() % pool.size()]);
    bad += check("random", keys);
    return bad ? 1 : 0;
}

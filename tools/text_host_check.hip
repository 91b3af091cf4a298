// text_host_check.hip -- dn_cov_text_host (csrc/dn_text.hip) under the host sanitizers, as a program of its own: nothing is
// loaded into Python and no device is touched.  The values of tests/_text_cases.py (ties, carries, signed zeros, subnormals,
// the largest doubles the rule covers) in the shapes of that file, a mixed batch with an empty gene, the flagged batch, and
// 20 000 seeded matrices go through the host entry from buffers of exactly their size -- the doubles without slack, so a
// read past a matrix is a read past the buffer -- and every piece is held to snprintf("%.5f"), byte for byte.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/text_host_check.hip degnorm_amd/csrc/dn_text.hip -o text_host_check && ./text_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the three functions below, so the unit links alone.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <limits>
#include <random>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

struct Gene {
    int64_t len;
    std::vector<double> v;          // p x len, row-major
    bool flagged;
};

static bool formattable(double x) { return x == x && fabs(x) < 9223372036854775808.0; }

// the piece of one gene as C prints it
static std::string expect(const Gene &g, int p)
{
    std::string s;
    char buf[64];
    for (int64_t j = 0; j < g.len; j++)
        for (int i = 0; i < p; i++) {
            snprintf(buf, sizeof(buf), "%.5f", g.v[(size_t) (i * g.len + j)]);
            s += buf;
            s += i + 1 < p ? ' ' : '\n';
        }
    return s;
}

static Gene gene_of(int p, int64_t len, const std::vector<double> &values, size_t first)
{
    Gene g{len, std::vector<double>((size_t) (p * len)), false};
    for (size_t k = 0; k < g.v.size(); k++) {
        g.v[k] = values[(first + k) % values.size()];
        if (!formattable(g.v[k])) g.flagged = true;
    }
    return g;
}

static int run(const char *name, int p, const std::vector<Gene> &genes)
{
    std::vector<double> x;                      // exactly the matrices
    std::vector<int64_t> beg, len;
    for (const Gene &g : genes) {
        beg.push_back((int64_t) x.size());
        len.push_back(g.len);
        x.insert(x.end(), g.v.begin(), g.v.end());
    }
    std::vector<int64_t> off(genes.size() + 1);
    std::vector<uint8_t> flag(genes.size());
    dn_text text = nullptr;
    const int rc = dn_cov_text_host(x.data(), (int64_t) x.size(), (int64_t) genes.size(), p, beg.data(), len.data(), off.data(), flag.data(), &text);
    if (rc != DN_OK) {
        fprintf(stderr, "%s: rc %d (%s)\n", name, rc, g_error.c_str());
        return 1;
    }
    int bad = 0;
    const uint8_t *bytes = dn_text_bytes(text);
    int64_t at = 0, n_flagged = 0;
    for (size_t k = 0; k < genes.size() && !bad; k++) {
        const std::string e = genes[k].flagged ? std::string() : expect(genes[k], p);
        n_flagged += genes[k].flagged;
        if (flag[k] != (genes[k].flagged ? 1 : 0) || off[k] != at || off[k + 1] - off[k] != (int64_t) e.size()
            || (e.size() && memcmp(bytes + at, e.data(), e.size()) != 0)) {
            fprintf(stderr, "%s: gene %zu differs (flag %d, piece %lld bytes at %lld, expected %zu at %lld)\n", name, k, flag[k],
                    (long long) (off[k + 1] - off[k]), (long long) off[k], e.size(), (long long) at);
            bad = 1;
        }
        at += (int64_t) e.size();
    }
    if (!bad && dn_text_size(text) != at) {
        fprintf(stderr, "%s: %lld bytes, expected %lld\n", name, (long long) dn_text_size(text), (long long) at);
        bad = 1;
    }
    dn_text_free(text);
    if (!bad) printf("%-16s %6zu genes, p = %3d, %10lld bytes, %lld flagged: ok\n", name, genes.size(), p, (long long) at, (long long) n_flagged);
    return bad;
}

static int refused(const char *name, int rc, const char *message)
{
    if (rc == DN_E_INVALID && g_error == message) {
        printf("%-16s refused: ok\n", name);
        return 0;
    }
    fprintf(stderr, "%s: rc %d (%s), expected \"%s\"\n", name, rc, g_error.c_str(), message);
    return 1;
}

int main()
{
    int bad = 0;
    std::mt19937_64 rng(20);
    std::vector<double> values;
    for (int k = 0; k < 4096; k++) {                               // ties: every multiple of 1/64 in [0, 64), both signs
        values.push_back(k / 64.0);
        values.push_back(-(k / 64.0));
    }
    for (int k = 1; k < 200000; k += 2) values.push_back(k * 5e-6);     // odd multiples of 5e-6
    const double special[] = {0.999995, 0.9999949999, 9.999999, 99999.999995, -0.0, -1e-9, 5e-324, 9007199254740991.0, 9007199254740993.0,
                              1e15 + 0.5, 4611686018427387904.0, nextafter(9223372036854775808.0, 0.0), 0.0, 1.0, 999999999.0, 1000000000.0,
                              999999999999999999.0, 1e18, 2.2250738585072014e-308, 0.5e-5, 1.5e-5, 2.5e-5};
    values.insert(values.end(), special, special + sizeof(special) / sizeof(special[0]));
    std::uniform_real_distribution<double> expo(-7.0, 11.0), unit(0.0, 1.0);
    for (int k = 0; k < 200000; k++) values.push_back((unit(rng) < 0.5 ? -1.0 : 1.0) * pow(10.0, expo(rng)) * (0.5 + unit(rng)));
    for (int k = 0; k < 5000; k++) values.push_back((double) (rng() % 5000));        // integer counts

    const int shapes[][2] = {{2, 1}, {2, 63}, {3, 64}, {3, 65}, {10, 257}, {64, 130}, {256, 70}};
    size_t first = 0;
    for (const auto &s : shapes) {
        // as many genes of the shape as walk all values once
        std::vector<Gene> genes;
        const size_t per = (size_t) s[0] * (size_t) s[1];
        for (size_t done = 0; done < values.size(); done += per, first += per) genes.push_back(gene_of(s[0], s[1], values, first));
        const std::string name = std::to_string(s[0]) + "x" + std::to_string(s[1]);
        bad += run(name.c_str(), s[0], genes);
    }
    {
        std::vector<Gene> genes;
        const int64_t lens[] = {1, 63, 700, 64, 0, 65, 257, 130, 70};
        for (int64_t L : lens) { genes.push_back(gene_of(3, L, values, first)); first += (size_t) (3 * L); }
        bad += run("mixed", 3, genes);
    }
    {
        std::vector<Gene> genes;
        for (int k = 0; k < 9; k++) { genes.push_back(gene_of(4, 40 + k, values, first)); first += 200; }
        const double inf = std::numeric_limits<double>::infinity();
        genes[1].v[7] = std::numeric_limits<double>::quiet_NaN(); genes[1].flagged = true;
        genes[3].v[0] = inf; genes[3].flagged = true;
        genes[4].v[genes[4].v.size() - 1] = -inf; genes[4].flagged = true;
        genes[8].v[50] = 9223372036854775808.0; genes[8].flagged = true;
        bad += run("flagged", 4, genes);
    }
    {
        std::vector<Gene> genes;
        std::uniform_int_distribution<int> len(0, 40);
        for (int k = 0; k < 20000; k++) {
            Gene g{len(rng), {}, false};
            g.v.resize((size_t) (5 * g.len));
            for (double &v : g.v) v = (unit(rng) < 0.3 ? -1.0 : 1.0) * pow(10.0, expo(rng)) * unit(rng);
            genes.push_back(g);
        }
        bad += run("seeded_20000", 5, genes);
    }
    // the refusals
    {
        const double x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        int64_t beg[2] = {0, 4}, len[2] = {2, 2}, off[3];
        uint8_t flag[2];
        dn_text text = nullptr;
        bad += refused("null", dn_cov_text_host(nullptr, 8, 2, 2, beg, len, off, flag, &text), "dn_cov_text_host: null argument");
        bad += refused("p_1", dn_cov_text_host(x, 8, 2, 1, beg, len, off, flag, &text), "dn_cov_text_host: fewer than 2 samples");
        len[1] = -1;
        bad += refused("negative", dn_cov_text_host(x, 8, 2, 2, beg, len, off, flag, &text), "dn_cov_text_host: gene 1 has a negative length");
        len[1] = 3;
        bad += refused("leaves", dn_cov_text_host(x, 8, 2, 2, beg, len, off, flag, &text), "dn_cov_text_host: gene 1 leaves the buffer");
        len[1] = 2; beg[1] = 3;
        bad += refused("overlap", dn_cov_text_host(x, 8, 2, 2, beg, len, off, flag, &text), "dn_cov_text_host: genes 0 and 1 overlap");
    }
    return bad ? 1 : 0;
}

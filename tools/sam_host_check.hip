// sam_host_check.hip -- dn_sam_encode_host (csrc/dn_sam.hip) under the host sanitizers, as a program of its own: nothing is
// loaded into Python and no device is touched.  Lines that reach every branch of the encoder (tests/_sam_cases.py has the
// same ones) go through the host entry from buffers of exactly their size -- text without slack, so a read past a line's end
// is a read past the buffer for the last line, and outputs of exactly the capacity the header promises to suffice -- and
// the result is held to what can be said without a second encoder: the count of records, offsets that ascend by
// 4 + block_size, the fixed fields of a known record, the float payloads, and for every malformed text its line and kind.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/sam_host_check.hip degnorm_amd/csrc/dn_sam.hip -o sam_host_check && ./sam_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the three functions below, so the unit links alone.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

static uint64_t fnv1a(const std::string &s)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : s) h = (h ^ c) * 0x100000001b3ull;
    return h;
}

struct Result {
    int rc;
    int64_t n_lines, n_rec, n_out, n_patch, err_line;
    int32_t err_kind;
    std::vector<uint8_t> out;
    std::vector<int64_t> off, patch;
};

static Result encode(const std::string &text)
{
    const std::vector<std::string> names = {"c1", "c2", "c3"};
    std::vector<int32_t> order = {0, 1, 2};
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return fnv1a(names[(size_t) a]) < fnv1a(names[(size_t) b]); });
    std::vector<uint64_t> hash;
    std::vector<int32_t> len;
    std::vector<int64_t> beg;
    std::vector<uint8_t> joined;
    for (int32_t k : order) {
        hash.push_back(fnv1a(names[(size_t) k]));
        beg.push_back((int64_t) joined.size());
        len.push_back((int32_t) names[(size_t) k].size());
        joined.insert(joined.end(), names[(size_t) k].begin(), names[(size_t) k].end());
    }
    const std::vector<uint8_t> bytes(text.begin(), text.end());          // exactly the text
    const int64_t n = (int64_t) bytes.size();
    const int64_t lines = (int64_t) std::count(text.begin(), text.end(), '\n') + 1;
    const int64_t floats = (int64_t) std::count(text.begin(), text.end(), ',') + (int64_t) std::count(text.begin(), text.end(), ':');
    Result r;
    r.out.resize((size_t) (2 * n + 36 * lines));
    r.off.resize((size_t) lines + 1);
    r.patch.resize((size_t) (2 * floats));
    r.rc = dn_sam_encode_host(bytes.data(), n, 3, hash.data(), order.data(), beg.data(), len.data(), joined.data(), (int64_t) joined.size(),
                              r.out.data(), (int64_t) r.out.size(), r.off.data(), (int64_t) r.off.size(), r.patch.data(), floats, &r.n_lines,
                              &r.n_rec, &r.n_out, &r.n_patch, &r.err_line, &r.err_kind);
    return r;
}

static std::string line(const std::string &qname = "r", const std::string &flag = "0", const std::string &rname = "c1", const std::string &pos = "100",
                        const std::string &mapq = "60", const std::string &cigar = "4M", const std::string &rnext = "*", const std::string &pnext = "0",
                        const std::string &tlen = "0", const std::string &seq = "ACGT", const std::string &qual = "IIII", const std::string &aux = "")
{
    return qname + "\t" + flag + "\t" + rname + "\t" + pos + "\t" + mapq + "\t" + cigar + "\t" + rnext + "\t" + pnext + "\t" + tlen + "\t" + seq + "\t"
           + qual + (aux.empty() ? "" : "\t" + aux);
}

static uint32_t le32(const uint8_t *p) { return (uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16 | (uint32_t) p[3] << 24; }

// a valid text of n_rec lines: DN_OK, no error, offsets that ascend by 4 + block_size up to n_out
static int valid(const char *name, const std::string &text, int64_t n_rec, int64_t n_patch)
{
    const Result r = encode(text);
    if (r.rc != DN_OK || r.err_kind != 0) {
        fprintf(stderr, "%s: rc %d (%s), error kind %d at line %lld\n", name, r.rc, g_error.c_str(), r.err_kind, (long long) r.err_line);
        return 1;
    }
    if (r.n_rec != n_rec || r.n_lines != n_rec || r.n_patch != n_patch || r.off[0] != 0 || r.off[(size_t) n_rec] != r.n_out) {
        fprintf(stderr, "%s: %lld records, %lld patches, expected %lld and %lld\n", name, (long long) r.n_rec, (long long) r.n_patch, (long long) n_rec,
                (long long) n_patch);
        return 1;
    }
    for (int64_t k = 0; k < n_rec; k++) {
        const int64_t o = r.off[(size_t) k], size = r.off[(size_t) k + 1] - o;
        if (size < 36 || (int64_t) le32(r.out.data() + o) != size - 4) {
            fprintf(stderr, "%s: record %lld of %lld bytes has block_size %u\n", name, (long long) k, (long long) size, le32(r.out.data() + o));
            return 1;
        }
    }
    for (int64_t k = 0; k < n_patch; k++)
        if (r.patch[(size_t) (2 * k)] < 0 || r.patch[(size_t) (2 * k)] + 4 > r.n_out || r.patch[(size_t) (2 * k + 1)] < 0
            || r.patch[(size_t) (2 * k + 1)] >= (int64_t) text.size()) {
            fprintf(stderr, "%s: patch entry %lld out of range\n", name, (long long) k);
            return 1;
        }
    printf("%-18s %6lld records, %8lld bytes, %3lld float payloads: ok\n", name, (long long) n_rec, (long long) r.n_out, (long long) n_patch);
    return 0;
}

static int faulty(const char *name, const std::string &text, int64_t err_line, int32_t err_kind)
{
    const Result r = encode(text);
    if (r.rc != DN_OK || r.err_line != err_line || r.err_kind != err_kind || r.n_rec != 0 || r.n_out != 0) {
        fprintf(stderr, "%s: rc %d (%s), kind %d at line %lld, expected kind %d at line %lld\n", name, r.rc, g_error.c_str(), r.err_kind,
                (long long) r.err_line, err_kind, (long long) err_line);
        return 1;
    }
    printf("%-18s kind %2d at line %lld: ok\n", name, err_kind, (long long) err_line);
    return 0;
}

template <class F> static std::string repeat(int n, F make)
{
    std::string s;
    for (int k = 0; k < n; k++) s += make(k);
    return s;
}

int main()
{
    int bad = 0;
    const std::string ok = line() + "\n";
    // one known record, byte for byte
    {
        const Result r = encode(line("r1", "16", "c2", "10", "7", "4M1I", "=", "20", "-7", "ACGTN", "IIII#", "NH:i:1\tXf:f:1.5") + "\n");
        const uint8_t expect[] = {62, 0, 0, 0, 1, 0, 0, 0, 9, 0, 0, 0, 3, 7, 0x49, 0x12, 2, 0, 16, 0, 5, 0, 0, 0, 1, 0, 0, 0, 19, 0, 0, 0, 0xf9, 0xff, 0xff, 0xff,
                                  'r', '1', 0, 0x40, 0, 0, 0, 0x11, 0, 0, 0, 0x12, 0x48, 0xf0, 40, 40, 40, 40, 2, 'N', 'H', 'C', 1, 'X', 'f', 'f', 0, 0, 0xc0, 0x3f};
        if (r.rc != DN_OK || r.n_out != (int64_t) sizeof(expect) || memcmp(r.out.data(), expect, sizeof(expect)) != 0) {
            fprintf(stderr, "known record: rc %d, %lld bytes\n", r.rc, (long long) r.n_out);
            bad++;
        } else {
            printf("%-18s byte for byte: ok\n", "known_record");
        }
    }
    bad += valid("one", ok, 1, 0);
    bad += valid("n257", repeat(257, [&](int k) { return line("q" + std::to_string(k), "0", k % 2 ? "c2" : "c3", std::to_string(1 + 7 * k)) + "\n"; }), 257, 0);
    bad += valid("no_final_newline", ok + line("b"), 2, 0);
    bad += valid("crlf", line("a") + "\r\n" + line("b") + "\r\n", 2, 0);
    bad += valid("long_line", ok + line("L", "0", "c1", "1", "0", "*", "*", "0", "0", std::string(16484, 'A'), "*") + "\n" + ok, 3, 0);
    bad += valid("names", line("n") + "\n" + line(std::string(254, 'N')) + "\n", 2, 0);
    bad += valid("seq_lengths", repeat(6, [&](int k) {
                     return line("s", "0", "c1", "1", "0", "*", "*", "0", "0", k ? std::string("acgtn=").substr(0, (size_t) k) : "*",
                                 k ? std::string("!~5Iab").substr(0, (size_t) k) : "*") + "\n"; }), 6, 0);
    bad += valid("qual_star", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "*") + "\n", 1, 0);
    bad += valid("cigar_star", line("r", "0", "*", "0", "0", "*", "*", "0", "0", "*", "*") + "\n", 1, 0);
    bad += valid("cigar_all_ops", line("r", "0", "c1", "1", "0", "1M2I3D4N5S6H7P8=9X", "*", "0", "0", std::string(25, 'A'), std::string(25, '#')) + "\n", 1, 0);
    bad += valid("cigar_65535", line("r", "0", "c1", "1", "0", repeat(32767, [](int) { return "1M1I"; }) + "1M", "*", "0", "0", std::string(65535, 'C'), "*") + "\n", 1, 0);
    bad += valid("extremes", line("r", "65535", "c1", "0", "255") + "\n" + line("r", "0", "c1", "2147483647", "0", "4M", "c3", "2147483647", "-2147483648") + "\n"
                                 + line("r", "0", "c1", "1", "0", "600000M", "=", "1", "2147483647", "*", "*") + "\n", 3, 0);
    bad += valid("tag_i", repeat(12, [&](int k) {
                     const char *v[] = {"-2147483648", "-32769", "-32768", "-129", "-128", "-1", "0", "255", "256", "65535", "65536", "4294967295"};
                     return line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", std::string("Xi:i:") + v[k]) + "\n"; }), 12, 0);
    bad += valid("tag_azh", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XA:A:x\tXZ:Z:hello world\tXe:Z:\tXH:H:1AE301\tXh:H:") + "\n", 1, 0);
    bad += valid("tag_b", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII",
                               "Xc:B:c\tXc:B:c,-128\tXC:B:C,255,0,7\tXs:B:s,-32768,32767,-1\tXS:B:S,65535\tXi:B:i,-2147483648,2147483647,5\tXI:B:I,4294967295\t"
                               "Xf:B:f\tXf:B:f,1.5\tXf:B:f,1.5,-0.25,1e-3") + "\n", 1, 4);
    // floats at the very end of the text, without a line end behind them
    bad += valid("tag_f", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "Xf:f:1.5\tXg:f:-0\tXh:f:.5\tXi:f:5.\tXj:f:1E+10\tXk:f:inf\tXl:f:-Infinity\tXn:f:1e-46") + "\n"
                               + line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XB:B:f,2,1.000000059604644776257986738"), 2, 10);

    bad += faulty("unknown_rname", ok + line("r", "0", "c9") + "\n", 2, DN_SAM_E_RNAME);
    bad += faulty("unknown_rnext", ok + line("r", "0", "c1", "1", "0", "4M", "c1x") + "\n", 2, DN_SAM_E_RNAME);
    bad += faulty("too_few_fields", ok + "r\t0\tc1\t1\t60\t4M\t*\t0\t0\tACGT\n", 2, DN_SAM_E_FIELDS);
    bad += faulty("one_field", "just words", 1, DN_SAM_E_FIELDS);
    bad += faulty("cut_in_flag", "r\t1", 1, DN_SAM_E_FIELDS);
    bad += faulty("bad_digit", ok + ok + line("r", "0", "c1", "1x") + "\n", 3, DN_SAM_E_INTEGER);
    bad += faulty("flag_range", line("r", "65536") + "\n", 1, DN_SAM_E_INTEGER);
    bad += faulty("pos_range", line("r", "0", "c1", "2147483648") + "\n", 1, DN_SAM_E_INTEGER);
    bad += faulty("long_integer", line("r", "0", "c1", "1234567890123456789") + "\n", 1, DN_SAM_E_INTEGER);
    bad += faulty("ops_65536", ok + line("r", "0", "c1", "1", "0", repeat(65536, [](int) { return "1M"; }), "*", "0", "0", "*", "*") + "\n", 2, DN_SAM_E_CIGAR_OPS);
    bad += faulty("bad_cigar", line("r", "0", "c1", "1", "0", "4Q") + "\n", 1, DN_SAM_E_CIGAR);
    bad += faulty("cigar_length", line("r", "0", "c1", "1", "0", "268435456M", "*", "0", "0", "*", "*") + "\n", 1, DN_SAM_E_CIGAR);
    bad += faulty("qual_length", ok + line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "III") + "\n", 2, DN_SAM_E_QUAL_LEN);
    bad += faulty("qual_byte", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "II I") + "\n", 1, DN_SAM_E_QUAL);
    bad += faulty("seq_cigar", line("r", "0", "c1", "1", "0", "5M") + "\n", 1, DN_SAM_E_SEQ_CIGAR);
    bad += faulty("name_255", ok + line(std::string(255, 'N')) + "\n", 2, DN_SAM_E_NAME);
    bad += faulty("i_above", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "Xi:i:4294967296") + "\n", 1, DN_SAM_E_TAG_RANGE);
    bad += faulty("i_below", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "Xi:i:-2147483649"), 1, DN_SAM_E_TAG_RANGE);
    bad += faulty("b_above", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XB:B:c,1,128"), 1, DN_SAM_E_TAG_ARRAY);
    bad += faulty("b_cut", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XB:B:i,1,"), 1, DN_SAM_E_TAG);
    bad += faulty("odd_h", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XH:H:1AE"), 1, DN_SAM_E_TAG_HEX);
    bad += faulty("bad_float", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "Xf:f:1e"), 1, DN_SAM_E_TAG_FLOAT);
    bad += faulty("short_tags", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XX:Z"), 1, DN_SAM_E_TAG);
    bad += faulty("tag_cut", line("r", "0", "c1", "1", "0", "4M", "*", "0", "0", "ACGT", "IIII", "XX:B:"), 1, DN_SAM_E_TAG);
    bad += faulty("empty_line", ok + "\n" + ok, 2, DN_SAM_E_EMPTY);
    bad += faulty("only_cr", "\r\n", 1, DN_SAM_E_EMPTY);
    return bad ? 1 : 0;
}

// gz_host_check.hip -- the host build of the gzip inflate (csrc/dn_gz.hip, dn_gz_open with device = -1) under the host sanitizers,
// as a program of its own: nothing is loaded into Python and no device is touched.  Seeded files that reach every branch of the
// definition (the cases of tests/_gz_cases.py, built here with the system's zlib) go through dn_gz_open / dn_gz_next from
// buffers of exactly their size -- a read past the compressed bytes is a read past the buffer -- at several chunk and span
// sizes, and must give the text they were made from, with the tables of a scan consistent with it.  Then 20 000 seeded
// mutations of a small file of many blocks: any status, the bytes of zlib's own inflate when both decode, and no report from
// a sanitizer.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/gz_host_check.hip degnorm_amd/csrc/dn_gz.hip -lz -o gz_host_check && ./gz_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the functions below, so the unit links alone.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

typedef std::vector<uint8_t> Bytes;

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static Bytes gtf_text(size_t min_bytes)
{
    std::string s;
    for (int g = 0; s.size() < min_bytes; g++) {
        const std::string id = "ENSG" + std::to_string(100000000 + g), chr = "chr" + std::to_string(1 + g % 22);
        uint64_t pos = 1000 + rnd() % 100000;
        for (int e = 0, n = 2 + (int) (rnd() % 10); e < n; e++) {
            const uint64_t len = 60 + rnd() % 900;
            s += chr + "\tHAVANA\texon\t" + std::to_string(pos) + "\t" + std::to_string(pos + len) + "\t.\t+\t.\tgene_id \"" + id +
                 "\"; gene_type \"protein_coding\"; gene_name \"GENE" + std::to_string(g) + "\"; exon_number " + std::to_string(e + 1) + ";\n";
            pos += len + 80 + rnd() % 4000;
        }
    }
    return Bytes(s.begin(), s.end());
}

static Bytes raw_deflate(const Bytes &plain, int level, int strategy, size_t sync_every)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(2); }
    Bytes out(deflateBound(&z, (uLong) plain.size()) + 64 + (sync_every ? 16 * (plain.size() / sync_every + 1) : 0));
    z.next_out = out.data(); z.avail_out = (uInt) out.size();
    size_t done = 0;
    while (sync_every && done + sync_every < plain.size()) {
        z.next_in = const_cast<Bytef *>(plain.data() + done); z.avail_in = (uInt) sync_every;
        deflate(&z, Z_SYNC_FLUSH);
        done += sync_every;
    }
    static uint8_t nothing = 0;
    z.next_in = plain.size() > done ? const_cast<Bytef *>(plain.data() + done) : &nothing; z.avail_in = (uInt) (plain.size() - done);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate failed\n"); exit(2); }
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

static void put32(Bytes &b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t) (v >> (8 * k))); }

static Bytes member(const Bytes &plain, int level = 6, int strategy = Z_DEFAULT_STRATEGY, size_t sync_every = 0, int flags = 0)
{
    Bytes m = {0x1f, 0x8b, 8, (uint8_t) flags, 0, 0, 0, 0, 0, 0xff};
    const auto add = [&m](const char *s, size_t n) { m.insert(m.end(), s, s + n); };
    if (flags & 4) add("\7\0AB\3\0xyz", 9);                                // XLEN 7: subfield AB of 3 bytes
    if (flags & 8) add("g.gtf", 6);
    if (flags & 16) add("seed", 5);
    if (flags & 2) { const uint32_t c = (uint32_t) crc32(0, m.data(), (uInt) m.size()); m.push_back((uint8_t) c); m.push_back((uint8_t) (c >> 8)); }
    const Bytes d = raw_deflate(plain, level, strategy, sync_every);
    m.insert(m.end(), d.begin(), d.end());
    put32(m, (uint32_t) crc32(0, plain.empty() ? nullptr : plain.data(), (uInt) plain.size()));
    put32(m, (uint32_t) plain.size());
    return m;
}

// rc of the first failing call (DN_OK: none); out = the bytes; tables checked for consistency when `tables`
static int gunzip(const Bytes &file, int64_t chunk, int64_t window, int verify, Bytes &out, bool tables = false)
{
    const Bytes comp(file.begin(), file.end());                              // exactly the file
    out.clear();
    dn_gz h = nullptr;
    int rc = dn_gz_open(comp.data(), (int64_t) comp.size(), -1, chunk, window, verify, 1, &h);
    if (rc != DN_OK) return rc;
    for (;;) {
        const uint8_t *p = nullptr;
        int64_t n = 0;
        int32_t done = 0;
        rc = dn_gz_next(h, &p, &n, &done);
        if (rc != DN_OK || done) break;
        out.insert(out.end(), p, p + n);
    }
    if (rc == DN_OK && tables) {
        int64_t c[DN_GZ_N_COUNTERS], n_chunks = 0, n_seg = 0, total = 0;
        const int64_t *guess = nullptr, *seg = nullptr;
        double ms[6];
        if (dn_gz_counters(h, c, ms) != DN_OK || dn_gz_tables(h, &n_chunks, &guess, &n_seg, &seg) != DN_OK) rc = -100;
        for (int64_t s = 0; s < n_seg && rc == DN_OK; s++) {
            total += seg[4 * s + 2];
            if (seg[4 * s] >= seg[4 * s + 1] || seg[4 * s + 1] > 8 * (int64_t) comp.size() || (s > 0 && seg[4 * s] < seg[4 * s - 3])) rc = -101;
        }
        for (int64_t k = 0; k < n_chunks && rc == DN_OK; k++)
            if (guess[k] != -1 && (guess[k] < 8 * k * chunk || guess[k] >= 8 * (k + 1) * chunk)) rc = -102;
        if (rc == DN_OK && (total != (int64_t) out.size() || c[6] != n_seg || c[1] != n_chunks || c[9] != total || c[3] + c[5] != c[6])) rc = -103;
    }
    dn_gz_close(h);
    return rc;
}

static int valid(const char *name, const Bytes &file, const Bytes &plain)
{
    const int64_t shapes[][2] = {{4096, 64 << 20}, {16384, 64 << 20}, {1 << 20, 64 << 20}, {4096, 65536}, {4096, 4096}};
    for (const auto &s : shapes) {
        Bytes out;
        const int rc = gunzip(file, s[0], s[1], 1, out, true);
        if (rc != DN_OK || out != plain) {
            fprintf(stderr, "%s (chunks of %lld, spans of %lld): rc %d (%s), %zu bytes, expected %zu\n", name, (long long) s[0], (long long) s[1], rc,
                    g_error.c_str(), out.size(), plain.size());
            return 1;
        }
    }
    printf("%-24s %8zu -> %8zu bytes: ok\n", name, file.size(), plain.size());
    return 0;
}

static int faulty(const char *name, const Bytes &file, const std::string &what)
{
    for (int64_t chunk : {4096, 1 << 20}) {
        Bytes out;
        const int rc = gunzip(file, chunk, 64 << 20, 1, out);
        if (rc != DN_E_INVALID || g_error != what) {
            fprintf(stderr, "%s: rc %d (%s), expected (%s)\n", name, rc, g_error.c_str(), what.c_str());
            return 1;
        }
    }
    printf("%-24s %s: ok\n", name, what.c_str());
    return 0;
}

static Bytes cat(const Bytes &a, const Bytes &b) { Bytes c(a); c.insert(c.end(), b.begin(), b.end()); return c; }

int main()
{
    int bad = 0;
    const Bytes text = gtf_text(1300000), small(text.begin(), text.begin() + 150000);
    for (int level : {1, 6, 9}) bad += valid(("text" + std::to_string(level)).c_str(), member(text, level), text);
    bad += valid("fixed", member(small, 6, Z_FIXED), small);
    bad += valid("huffman_only", member(small, 6, Z_HUFFMAN_ONLY), small);
    bad += valid("rle", member(small, 6, Z_RLE), small);
    bad += valid("stored", member(small, 0), small);
    bad += valid("empty", member(Bytes()), Bytes());
    bad += valid("no_bytes", Bytes(), Bytes());
    bad += valid("one_byte", member(Bytes(1, 'x')), Bytes(1, 'x'));
    bad += valid("m32768", member(Bytes(text.begin(), text.begin() + 32768)), Bytes(text.begin(), text.begin() + 32768));
    bad += valid("m32769", member(Bytes(text.begin(), text.begin() + 32769)), Bytes(text.begin(), text.begin() + 32769));
    {
        Bytes block(32768), six;
        for (uint8_t &b : block) b = (uint8_t) rnd();
        for (int k = 0; k < 6; k++) six.insert(six.end(), block.begin(), block.end());
        bad += valid("long_refs", member(six), six);
    }
    bad += valid("run", member(Bytes(1 << 20, 0), 0), Bytes(1 << 20, 0));
    bad += valid("run6", member(Bytes(1 << 20, 'A'), 6), Bytes(1 << 20, 'A'));
    bad += valid("sync_flush", member(text, 6, Z_DEFAULT_STRATEGY, 50000), text);
    bad += valid("nested", member(member(text, 6), 0), member(text, 6));
    {
        const Bytes a(small.begin(), small.begin() + 70000), b(small.begin() + 70000, small.end());
        bad += valid("three_members", cat(cat(member(a), member(Bytes())), member(b)), small);
    }
    bad += valid("header_fields", member(small, 6, Z_DEFAULT_STRATEGY, 0, 4 | 8 | 16 | 2), small);
    bad += valid("zero_padding", cat(member(small), Bytes(300, 0)), small);

    const Bytes z = member(small);
    bad += faulty("cut_header", Bytes(z.begin(), z.begin() + 5), "gzip member at byte 0: truncated header");
    bad += faulty("cut_stream", Bytes(z.begin(), z.begin() + z.size() / 2), "gzip member at byte 0: truncated deflate stream");
    bad += faulty("cut_trailer", Bytes(z.begin(), z.end() - 3), "gzip member at byte 0: truncated trailer");
    { Bytes m = z; m[1] = 0x8c; bad += faulty("bad_magic", m, "gzip member at byte 0: bad magic"); }
    { Bytes m = z; m[2] = 7; bad += faulty("cm_7", m, "gzip member at byte 0: compression method 7"); }
    { Bytes m = z; m[3] = 0x20; bad += faulty("reserved_flag", m, "gzip member at byte 0: reserved flag bits set"); }
    { Bytes m = member(small, 0); m[10 + 5 + 7000] ^= 0x10; bad += faulty("stored_bit_flip", m, "gzip member at byte 0: CRC32 mismatch"); }
    { Bytes m = z; m[m.size() - 4] ^= 1; bad += faulty("wrong_isize", m, "gzip member at byte 0: ISIZE mismatch"); }
    // the next entry is bit 8 n of a file whose size n is a multiple of the chunk: a header, or a block that is not final, ends it
    const auto padded_header = [](size_t total) {                            // a member header of `total` bytes: FEXTRA fills it
        Bytes h = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff};
        const size_t xlen = total - 12;
        for (size_t v : {xlen & 0xff, xlen >> 8, (size_t) 'A', (size_t) 'B', (xlen - 4) & 0xff, (xlen - 4) >> 8}) h.push_back((uint8_t) v);
        h.resize(total, 0);
        return h;
    };
    bad += faulty("header_ends_file", padded_header(4096), "gzip member at byte 0: truncated deflate stream");
    bad += faulty("second_header_ends_file", cat(z, padded_header(8192 - z.size() % 4096)),
                  "gzip member at byte " + std::to_string(z.size()) + ": truncated deflate stream");
    {
        Bytes d = raw_deflate(small, 6, Z_DEFAULT_STRATEGY, 50000);
        size_t end = 0;                                                      // behind the first sync flush: 00 00 ff ff, byte-aligned
        for (size_t k = 4; k <= d.size() && !end; k++)
            if (d[k - 4] == 0 && d[k - 3] == 0 && d[k - 2] == 0xff && d[k - 1] == 0xff) end = k;
        d.resize(end);
        bad += faulty("cut_behind_sync_flush", cat(padded_header(8192 - end % 4096), d), "gzip member at byte 0: truncated deflate stream");
    }
    bad += faulty("trailing_garbage", cat(z, Bytes(3, 'g')), "gzip member at byte " + std::to_string(z.size()) + ": trailing garbage");

    // seeded damage to a file of many small blocks, read in chunks and spans of 4 KiB
    {
        const Bytes base = member(Bytes(text.begin(), text.begin() + 120000), 6, Z_DEFAULT_STRATEGY, 6000);
        int64_t decoded = 0, errors = 0;
        for (int k = 0; k < 20000 && !bad; k++) {
            Bytes m = base;
            for (int n = 1 + (int) (rnd() % 2); n > 0; n--) {
                const size_t p = 10 + (size_t) (rnd() % (m.size() - 10));
                if (rnd() % 8) m[p] ^= (uint8_t) (1u << (rnd() % 8));
                else m.erase(m.begin() + (long) p, m.begin() + (long) std::min(m.size(), p + (size_t) (rnd() % 40)));
            }
            Bytes out;
            const int rc = gunzip(m, 4096, k % 2 ? 4096 : 64 << 20, 0, out);
            if (rc != DN_OK && rc != DN_E_INVALID) { fprintf(stderr, "mutation %d: rc %d (%s)\n", k, rc, g_error.c_str()); bad++; break; }
            Bytes ref(4 << 20);
            z_stream s;
            memset(&s, 0, sizeof s);
            inflateInit2(&s, -15);
            s.next_in = m.data() + 10; s.avail_in = (uInt) (m.size() - 10);
            s.next_out = ref.data(); s.avail_out = (uInt) ref.size();
            const int zrc = inflate(&s, Z_FINISH);
            const bool zok = zrc == Z_STREAM_END && s.avail_in == 8 && (uint32_t) s.total_out == (uint32_t) (m[m.size() - 4] | (m[m.size() - 3] << 8) |
                                                                                                           (m[m.size() - 2] << 16) | ((uint32_t) m[m.size() - 1] << 24));
            const bool full = s.avail_out == 0;
            ref.resize(s.total_out);
            inflateEnd(&s);
            if (full) continue;                                         // more than the text could ever be: not compared
            if (zok != (rc == DN_OK) || (zok && ref != out)) {
                fprintf(stderr, "mutation %d: zlib %s (%d), here rc %d (%s), %zu against %zu bytes\n", k, zok ? "decodes" : "fails", zrc, rc, g_error.c_str(),
                        ref.size(), out.size());
                bad++;
                break;
            }
            if (rc == DN_OK) decoded++; else errors++;
        }
        printf("%-24s %lld decoded as zlib does, %lld with an error: ok\n", "mutations", (long long) decoded, (long long) errors);
    }
    return bad ? 1 : 0;
}

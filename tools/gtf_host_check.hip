// gtf_host_check.hip -- the GTF rule of a line (dn::gtf::parse_line, csrc/dn_gtf.hpp) under the host sanitizers, as a program
// of its own: nothing is loaded into Python and no device is touched.  The device runs the rule on Bytes, which reads a
// padded buffer and so hides a read past a line's end; here it runs on HostText from buffers of exactly the text's size --
// text without slack, so such a read is a read past the buffer for the last line.  The texts are those of
// tests/test_gpu_annotation.py (BAD, EDGES and the features its docstring lists); each is split into lines as the scanner
// splits it, and the rows or the first error are held to what the text is written to show.  Then 20 000 seeded mutations of
// a small file: any status, but no report from a sanitizer.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/gtf_host_check.hip -o gtf_host_check && ./gtf_host_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_gtf.hpp"

struct Row {
    int64_t line;
    std::string chr;
    int64_t start, end;
    std::string gene;
    bool operator==(const Row &o) const { return line == o.line && chr == o.chr && start == o.start && end == o.end && gene == o.gene; }
};

struct Result {
    int64_t n_lines = 0, err_line = 0;
    int err_kind = 0;
    bool inside = true;                 // every span lies inside its line
    std::vector<Row> rows;
};

// the scanner's split: a line ends at '\n' or at the end of the bytes, and no line stands behind a final '\n'
static Result scan(const std::string &text)
{
    const std::vector<uint8_t> bytes(text.begin(), text.end());          // exactly the text
    const int64_t n = (int64_t) bytes.size();
    dn::HostText in{bytes.data()};
    Result r;
    for (int64_t pos = 0; pos < n; r.n_lines++) {
        const uint8_t *nl = (const uint8_t *) memchr(bytes.data() + pos, '\n', (size_t) (n - pos));
        const int64_t stop = nl ? (int64_t) (nl - bytes.data()) : n;
        int64_t chr_end = 0, start = 0, end = 0, g_lo = 0, g_hi = 0;
        const int k = dn::gtf::parse_line(in, pos, stop, &chr_end, &start, &end, &g_lo, &g_hi);
        if (k < 0 && !r.err_kind) { r.err_line = r.n_lines + 1; r.err_kind = -k; }
        if (k == dn::kExon) {
            if (chr_end < pos || chr_end > stop || g_lo < pos || g_hi < g_lo || g_hi > stop) { r.inside = false; return r; }
            r.rows.push_back(Row{r.n_lines + 1, text.substr((size_t) pos, (size_t) (chr_end - pos)), start, end, text.substr((size_t) g_lo, (size_t) (g_hi - g_lo))});
        }
        pos = stop + 1;
    }
    return r;
}

static std::string ln(const std::string &chr, const std::string &kind, const std::string &a, const std::string &b, const std::string &attrs)
{
    return chr + "\ttest\t" + kind + "\t" + a + "\t" + b + "\t.\t+\t.\t" + attrs;
}

static int valid(const char *name, const std::string &text, int64_t n_lines, const std::vector<Row> &rows)
{
    const Result r = scan(text);
    if (!r.inside || r.err_kind || r.n_lines != n_lines || !(r.rows == rows)) {
        fprintf(stderr, "%s: kind %d at line %lld, %lld lines (expected %lld), %zu rows (expected %zu)%s\n", name, r.err_kind, (long long) r.err_line,
                (long long) r.n_lines, (long long) n_lines, r.rows.size(), rows.size(), r.inside ? "" : ", a span outside its line");
        for (const Row &x : r.rows) fprintf(stderr, "    %lld %s %lld %lld [%s]\n", (long long) x.line, x.chr.c_str(), (long long) x.start, (long long) x.end, x.gene.c_str());
        return 1;
    }
    printf("%-34s %4zu rows: ok\n", name, rows.size());
    return 0;
}

static int faulty(const char *name, const std::string &text, int64_t err_line, int err_kind)
{
    const Result r = scan(text);
    if (!r.inside || r.err_line != err_line || r.err_kind != err_kind) {
        fprintf(stderr, "%s: kind %d at line %lld, expected kind %d at line %lld\n", name, r.err_kind, (long long) r.err_line, err_kind, (long long) err_line);
        return 1;
    }
    printf("%-34s kind %d at line %lld: ok\n", name, err_kind, (long long) err_line);
    return 0;
}

int main()
{
    int bad = 0;
    const std::string exon = "chr1\ttest\texon\t101\t300\t.\t+\t.\t";
    const auto row = [](int64_t line, const char *gene) { return Row{line, "chr1", 101, 300, gene}; };

    // what the docstring of tests/test_gpu_annotation.py lists
    bad += valid("name_before_id", exon + "gene_name \"N1\"; gene_id \"I1\";\n", 1, {row(1, "N1")});
    bad += valid("name_after_id", exon + "gene_id \"I1\"; transcript_id \"T\"; gene_name \"N1\";\n", 1, {row(1, "N1")});
    bad += valid("id_alone", exon + "gene_id \"I1\"; transcript_id \"T\";\n", 1, {row(1, "I1")});
    bad += valid("empty_name_falls_to_id", exon + "gene_name \"\"; gene_id \"I1\";\n" + exon + "gene_id \"I2\"; gene_name \" \";\n", 2, {row(1, "I1"), row(2, "I2")});
    bad += valid("second_name_is_not_read", exon + "gene_name \"\"; gene_name \"N2\"; gene_id \"I1\";\n", 1, {row(1, "I1")});
    bad += valid("exon_in_any_case", ln("1", "Exon", "5", "9", "gene_id \"A\";") + "\n" + ln("X", "EXON", "6", "7", "gene_id \"B\";") + "\n"
                                     + ln("1", "exons", "5", "9", "gene_id \"C\";") + "\n" + ln("1", "exo", "5", "9", "") + "\n",
                 4, {Row{1, "1", 5, 9, "A"}, Row{2, "X", 6, 7, "B"}});
    bad += valid("other_features", ln("chr1", "gene", ".", "NA", "note \"no gene tag\";") + "\n" + ln("chr1", "CDS", "1", "2", "") + "\n"
                                   + ln("chr1", "transcript", "1", "2", "gene_id \"A\"") + "\n" + exon + "gene_id \"A\";\n", 4, {row(4, "A")});
    bad += valid("no_trailing_semicolon", exon + "gene_id \"I1\"; gene_name \"N1\"\n" + exon + "gene_name N2\n", 2, {row(1, "N1"), row(2, "N2")});
    bad += valid("blanks_around_semicolons", exon + "  transcript_id \"T\"  ;   gene_name   \"N 1\"   ;  gene_id \"I1\" ;  \n", 1, {row(1, "N 1")});
    bad += valid("tenth_field", exon + "gene_id \"I1\"\tgene_name \"N1\";\n", 1, {row(1, "I1")});
    bad += valid("crlf", "##header\r\n\r\n" + exon + "gene_id \"A\";\r\n" + exon + "gene_name \"B\"\r\n", 4, {row(3, "A"), row(4, "B")});
    bad += valid("last_line_without_newline", exon + "gene_id \"A\";\n" + exon + "gene_id \"B\"", 2, {row(1, "A"), row(2, "B")});
    bad += valid("big_integers", ln("c", "exon", std::string(17, '0') + "7", std::string(18, '9'), "gene_id G") + "\n", 1,
                 {Row{1, "c", 7, 999999999999999999ll, "G"}});
    bad += valid("empty_chromosome", ln("", "exon", "1", "2", "gene_id G"), 1, {Row{1, "", 1, 2, "G"}});

    // EDGES
    bad += valid("newlines_only", "\n\n\n\n", 4, {});
    bad += valid("one_comment_no_newline", "#only a comment", 1, {});
    bad += valid("crlf_blanks", "\r\n#x\r\n\r\n", 3, {});
    bad += valid("one_line_no_newline", exon + "gene_id \"A\"", 1, {row(1, "A")});
    bad += valid("one_line_ending_in_cr", exon + "gene_id \"A\"\r", 1, {row(1, "A")});
    bad += valid("one_crlf_line", exon + "gene_id \"A\"\r\n", 1, {row(1, "A")});
    bad += valid("blank_lines_over_several_tiles", std::string(70000, '\n') + exon + "gene_name A;" + std::string(70000, '\n'), 140000, {row(70001, "A")});
    bad += valid("a_300_KB_line", exon + std::string(300000, ';') + "gene_name \"far away\"", 1, {row(1, "far away")});
    bad += valid("a_lone_cr", "\r", 1, {});

    // BAD: as the first line, in the middle and as the last line of valid lines, with and without a final newline; a second
    // faulty line behind it is not the one reported
    const struct { const char *name; std::string line; int kind; } faults[] = {
        {"fields_five", "chr1\ttest\tgene\t101\t300", DN_GTF_E_FIELDS},
        {"fields_eight", "chr1\ttest\texon\t101\t300\t.\t+\t.", DN_GTF_E_FIELDS},
        {"fields_no_tabs", "just some text", DN_GTF_E_FIELDS},
        {"gene_no_tag", exon + "transcript_id \"T1\"; exon_number 1;", DN_GTF_E_GENE},
        {"gene_empty_values", exon + "gene_name \"\"; gene_id \" \";", DN_GTF_E_GENE},
        {"gene_no_attributes", exon, DN_GTF_E_GENE},
        {"integer_letter", "chr1\ttest\texon\t10a\t300\t.\t+\t.\tgene_id \"A\";", DN_GTF_E_INTEGER},
        {"integer_empty", "chr1\ttest\tEXON\t101\t\t.\t+\t.\tgene_id \"A\";", DN_GTF_E_INTEGER},
        {"integer_exponent", "chr1\ttest\texon\t1e3\t3000\t.\t+\t.\tgene_id \"A\";", DN_GTF_E_INTEGER},
        {"integer_sign", "chr1\ttest\texon\t-5\t300\t.\t+\t.\tgene_id \"A\";", DN_GTF_E_INTEGER},
        {"integer_19_digits", ln("c", "exon", "1", std::string(19, '1'), "gene_id G"), DN_GTF_E_INTEGER}};
    std::vector<std::string> good;
    for (int k = 0; k < 30; k++) good.push_back(ln("chr1", k % 3 ? "exon" : "gene", std::to_string(10 * k + 1), std::to_string(10 * k + 9), "gene_id \"ID_G\"; gene_name \"G\";"));
    for (const auto &f : faults)
        for (size_t at : {(size_t) 0, (size_t) 17, good.size()})
            for (const char *tail : {"\n", ""}) {
                std::string text;
                for (size_t k = 0; k < at; k++) text += good[k] + "\n";
                text += f.line + "\n";
                for (size_t k = at; k < good.size(); k++) text += good[k] + "\n";
                text += f.line + tail;
                bad += faulty((std::string(f.name) + "@" + std::to_string(at + 1) + (*tail ? "" : ", open")).c_str(), text, (int64_t) at + 1, f.kind);
            }

    // seeded damage: a byte replaced, often by one that matters to the rule, or a stretch cut out
    {
        std::string base = "##description: small\n";
        for (int g = 0; g < 8; g++) {
            const std::string k = std::to_string(g);
            base += ln("chr" + k, "gene", "1", "90", "gene_id \"ID" + k + "\"; gene_name \"G" + k + "\";") + "\n";
            base += ln("chr" + k, "exon", "1", "9", "gene_id \"ID" + k + "\"; transcript_id \"T\"; gene_name \"G" + k + "\"; exon_number 1;") + (g % 2 ? "\r\n" : "\n");
            base += ln("chr" + k, "Exon", "11", "19", g % 3 ? "gene_name \"\"; gene_id ID" + k : " gene_name  N" + k + " ;") + "\n";
        }
        const std::string special("\t\n\r;\" #gen_idam0eE\0\xff", 21);
        uint64_t s = 0x9e3779b97f4a7c15ull;
        const auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        int64_t rows = 0, errors = 0;
        for (int k = 0; k < 20000; k++) {
            std::string t = base;
            for (int m = (int) (next() % 3) + 1; m > 0 && !t.empty(); m--) {
                const size_t p = (size_t) (next() % t.size());
                const int what = (int) (next() % 4);
                if (what == 0) t[p] = (char) (next() & 0xff);
                else if (what < 3) t[p] = special[(size_t) (next() % special.size())];
                else t.erase(p, (size_t) (next() % 60));
            }
            const Result r = scan(t);
            if (!r.inside) { fprintf(stderr, "mutation %d: a span outside its line\n", k); bad++; break; }
            if (r.err_kind) errors++; else rows++;
        }
        printf("%-34s %lld with rows, %lld with an error: ok\n", "mutations", (long long) rows, (long long) errors);
    }
    return bad ? 1 : 0;
}

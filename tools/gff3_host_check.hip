// gff3_host_check.hip -- dn_gff3_scan_host (csrc/dn_gff3.hip) under the host sanitizers, as a program of its own: nothing is
// loaded into Python and no device is touched.  Texts that reach every branch of the rule (tests/_gff3_fixtures.py has the
// same ones) go through the host entry from buffers of exactly their size -- text without slack, so a read past a line's end
// is a read past the buffer for the last line, and outputs of exactly the capacity the header promises to suffice -- with
// full and with 4-bit ID hashes, and the result is held to what each text is written to show: the gene of every exon line, or
// the line and kind of the error.  Then 20 000 seeded mutations of a small file: any status, but no report from a sanitizer.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/gff3_host_check.hip degnorm_amd/csrc/dn_gff3.hip -o gff3_host_check && ./gff3_host_check
//
// The error channel of the library (dn_api.hip) is replaced by the three functions below, so the unit links alone.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../include/degnorm_amd.h"
#include "../degnorm_amd/csrc/dn_host.hpp"

static std::string g_error;
int dn::fail(int code, const std::string &msg) { g_error = msg; return code; }
int dn::fail_hip(const char *what, hipError_t) { g_error = what; return DN_E_HIP; }
void dn::clear_error() { g_error.clear(); }

struct Result {
    int rc;
    int64_t n_lines, n_rows, n_nodes, n_walked, err_line;
    int32_t err_kind;
    std::vector<std::string> genes, chrs;
    std::vector<int64_t> line, start, end;
};

static Result scan(const std::string &text, int32_t hash_bits)
{
    const std::vector<uint8_t> bytes(text.begin(), text.end());          // exactly the text
    const int64_t n = (int64_t) bytes.size(), cap = n / 20 + 1;
    std::vector<int64_t> line((size_t) cap), c_beg((size_t) cap), start((size_t) cap), end((size_t) cap), g_beg((size_t) cap);
    std::vector<int32_t> c_len((size_t) cap), g_len((size_t) cap);
    std::vector<uint64_t> c_hash((size_t) cap), g_hash((size_t) cap);
    Result r;
    r.rc = dn_gff3_scan_host(bytes.data(), n, hash_bits, cap, &r.n_lines, &r.n_rows, line.data(), c_beg.data(), c_len.data(), c_hash.data(), start.data(),
                             end.data(), g_beg.data(), g_len.data(), g_hash.data(), &r.n_nodes, &r.n_walked, &r.err_line, &r.err_kind);
    if (r.rc != DN_OK) return r;
    for (int64_t k = 0; k < r.n_rows; k++) {
        const size_t i = (size_t) k;
        if (c_beg[i] < 0 || c_len[i] < 0 || c_beg[i] + c_len[i] > n || g_beg[i] < 0 || g_len[i] < 0 || g_beg[i] + g_len[i] > n) {
            r.rc = -100;                                                    // a span outside the text
            return r;
        }
        r.chrs.push_back(text.substr((size_t) c_beg[i], (size_t) c_len[i]));
        r.genes.push_back(text.substr((size_t) g_beg[i], (size_t) g_len[i]));
        r.line.push_back(line[i]); r.start.push_back(start[i]); r.end.push_back(end[i]);
    }
    return r;
}

static std::string ln(const std::string &chr, const std::string &kind, const std::string &a, const std::string &b, const std::string &attrs)
{
    return chr + "\tsrc\t" + kind + "\t" + a + "\t" + b + "\t.\t+\t.\t" + attrs;
}

static std::string joined(const std::vector<std::string> &lines, const std::string &nl = "\n", bool last = true)
{
    std::string s;
    for (size_t k = 0; k < lines.size(); k++) s += lines[k] + (k + 1 < lines.size() || last ? nl : "");
    return s;
}

static int valid(const char *name, const std::string &text, const std::vector<std::string> &genes)
{
    for (int32_t bits : {64, 4, 1}) {
        const Result r = scan(text, bits);
        bool ok = r.rc == DN_OK && r.err_kind == 0 && r.genes == genes;
        if (!ok) {
            fprintf(stderr, "%s (%d bits): rc %d (%s), kind %d at line %lld, %lld rows, expected %zu\n", name, bits, r.rc, g_error.c_str(), r.err_kind,
                    (long long) r.err_line, (long long) r.n_rows, genes.size());
            for (const std::string &g : r.genes) fprintf(stderr, "    %s\n", g.c_str());
            return 1;
        }
    }
    printf("%-34s %4zu rows: ok\n", name, genes.size());
    return 0;
}

static int faulty(const char *name, const std::string &text, int64_t err_line, int32_t err_kind)
{
    for (int32_t bits : {64, 4}) {
        const Result r = scan(text, bits);
        if (r.rc != DN_OK || r.err_line != err_line || r.err_kind != err_kind || r.n_rows != 0) {
            fprintf(stderr, "%s (%d bits): rc %d (%s), kind %d at line %lld, expected kind %d at line %lld\n", name, bits, r.rc, g_error.c_str(), r.err_kind,
                    (long long) r.err_line, err_kind, (long long) err_line);
            return 1;
        }
    }
    printf("%-34s kind %d at line %lld: ok\n", name, err_kind, (long long) err_line);
    return 0;
}

static std::string chain(int n)
{
    std::vector<std::string> out = {ln("c1", "exon", "10", "20", "Parent=n1")};
    for (int k = 1; k < n; k++) out.push_back(ln("c1", "region", "1", "100", "ID=n" + std::to_string(k) + ";Parent=n" + std::to_string(k + 1)));
    out.push_back(ln("c1", "gene", "1", "100", "ID=n" + std::to_string(n) + ";Name=TOP"));
    return joined(out);
}

int main()
{
    int bad = 0;
    const std::string gene = ln("c1", "gene", "1", "500", "ID=gene:G1;Name=ALPHA;gene_id=G1");
    const std::string tx = ln("c1", "mRNA", "1", "500", "ID=transcript:T1;Parent=gene:G1;Name=ALPHA-201");
    const std::string ex = ln("c1", "exon", "10", "90", "Parent=transcript:T1;Name=E1");
    const std::string own = ln("c2", "exon", "5", "50", "ID=e9;gene_name=OWN");
    // one known row, field for field
    {
        const Result r = scan(joined({"##gff-version 3", gene, tx, ex}), 64);
        if (r.rc != DN_OK || r.n_lines != 4 || r.n_rows != 1 || r.n_nodes != 2 || r.n_walked != 1 || r.line[0] != 4 || r.chrs[0] != "c1" || r.start[0] != 10
            || r.end[0] != 90 || r.genes[0] != "ALPHA") {
            fprintf(stderr, "known row: rc %d, %lld rows\n", r.rc, (long long) r.n_rows);
            bad++;
        } else {
            printf("%-34s field for field: ok\n", "known_row");
        }
    }
    bad += valid("one_line", own, {"OWN"});
    bad += valid("no_final_newline", joined({gene, tx, ex}, "\n", false), {"ALPHA"});
    bad += valid("headers_blank_crlf", joined({"##gff-version 3", "", "#!x", gene, "", tx, "###", ex, "", own}, "\r\n"), {"ALPHA", "OWN"});
    bad += valid("fasta_tail", joined({gene, tx, ex, "##FASTA", ">c1", "ACGT\tACGT", "c1\tx\texon\tq\t2\t.\t+\t.\tgene=Z", ln("c1", "exon", "1", "2", "Parent=nobody"),
                                       "ACGTACGT"}), {"ALPHA"});
    bad += valid("fasta_crlf_first", "##FASTA\r\n>c1\r\nACGT\r\n", {});
    bad += valid("not_quite_fasta", joined({"##FASTA ", "##fasta", "###FASTA", own}), {"OWN"});
    bad += valid("children_first", joined({ex, ln("c1", "EXON", "100", "190", "Parent=transcript:T1"), tx, gene}), {"ALPHA", "ALPHA"});
    bad += valid("several_parents", joined({gene, tx, ln("c1", "gene", "1", "9", "ID=gene:G2;Name=BETA"), ln("c1", "mRNA", "1", "9", "ID=transcript:T9;Parent=gene:G2"),
                                            ln("c1", "exon", "10", "90", "Parent=transcript:T9,transcript:T1"),
                                            ln("c1", "exon", "10", "91", "Parent= transcript:T1 , transcript:T9"),
                                            ln("c1", "exon", "10", "92", "Parent=,transcript:T1;gene_id=FALLBACK")}), {"BETA", "ALPHA", "FALLBACK"});
    bad += valid("repeated_ids", joined({ln("c1", "CDS", "1", "9", "ID=dup;Name=FIRST"), ln("c1", "CDS", "20", "29", "ID=dup;Name=SECOND"),
                                         ln("c1", "exon", "1", "9", "Parent=dup"), ln("c1", "CDS", "40", "49", "ID=dup;gene=THIRD")}), {"FIRST"});
    bad += valid("spaces", joined({ln("c1", "gene", "1", "9", " ID = g 1 ; Name =  SPACED NAME  ;"), ln("c1", "exon", "1", "9", " Parent = g 1 ;; x"),
                                   ln("c1", "exon", "2", "9", "note=a=b; gene_name = A=B ")}), {"SPACED NAME", "A=B"});
    bad += valid("empty_values", joined({ln("c1", "gene", "1", "9", "ID=g1;gene_name=;gene=;Name=;gene_id=GID"), ln("c1", "exon", "1", "9", "gene_name=;gene=;Parent=g1"),
                                         ln("c1", "gene", "1", "9", "ID=g2;Name=;gene_id="), ln("c1", "exon", "2", "9", "gene_name;Parent=g2"),
                                         ln("c1", "exon", "3", "9", "gene_name=;gene_name=SECOND;gene_id=THIRD"), ln("c1", "gene", "1", "9", "ID=;Name=NOID"),
                                         ln("c1", "exon", "4", "9", "Parent=;gene_id=X")}), {"GID", "g2", "THIRD", "X"});
    bad += valid("gene_against_gene_id", joined({ln("c1", "exon", "1", "9", "gene_id=ID1;Gene=no;GENE=no;gene_names=no;gene=YES"), ln("c1", "exon", "2", "9", "gene_id=ID2;xgene=no"),
                                                 ln("c1", "gene", "1", "9", "ID=g;gene_id=GID;name=no;Name=RN"),
                                                 ln("c1", "exon", "3", "9", "gene_id=ID3;Parent=g;parent=no;id=no")}), {"YES", "ID2", "RN"});
    bad += valid("chain_8", chain(8), {"TOP"});
    bad += valid("tenth_field", ln("c1", "gene", "1", "9", "ID=g;Name=N\tgene=EXTRA") + "\n" + ln("c1", "exon", "1", "9", "Parent=g\tgene=EXTRA\tmore") + "\n", {"N"});
    bad += valid("attributes_end_the_text", ln("c1", "gene", "1", "9", "ID=g;Name=N") + "\n" + ln("c1", "exon", "1", "9", "Parent=g"), {"N"});
    bad += valid("tag_ends_the_text", ln("c1", "exon", "1", "9", "gene_id=G;Parent"), {"G"});
    bad += valid("equals_ends_the_text", ln("c1", "exon", "1", "9", "gene=G;Parent="), {"G"});
    bad += valid("long_line", joined({gene, ln("c1", "mRNA", "1", "500", "ID=transcript:T2;Parent=gene:G1;Note=" + std::string(70000, 'x')),
                                      ln("c1", "exon", "10", "90", "Parent=transcript:T2")}), {"ALPHA"});
    bad += valid("big_integers", ln("c1", "exon", std::string(17, '0') + "7", std::string(18, '9'), "gene=G") + "\n", {"G"});

    bad += faulty("few_fields", joined({gene, "c1\tsrc\texon\t1\t2\t.\t+\t."}), 2, DN_GFF3_E_FIELDS);
    bad += faulty("no_tabs", "just words", 1, DN_GFF3_E_FIELDS);
    bad += faulty("cut_in_start", "c1\tsrc\texon\t1", 1, DN_GFF3_E_FIELDS);
    bad += faulty("bad_start", joined({gene, tx, ln("c1", "exon", "1x", "9", "gene=G")}), 3, DN_GFF3_E_INTEGER);
    bad += faulty("empty_end", ln("c1", "exon", "1", "", "gene=G") + "\n", 1, DN_GFF3_E_INTEGER);
    bad += faulty("long_integer", ln("c1", "exon", "1", std::string(19, '1'), "gene=G"), 1, DN_GFF3_E_INTEGER);
    bad += faulty("nothing_usable", joined({gene, ln("c1", "exon", "1", "9", "ID=e1;Name=E;gene_name=;gene_id=;Parent=")}), 2, DN_GFF3_E_GENE);
    bad += faulty("empty_attributes", ln("c1", "exon", "1", "9", ""), 1, DN_GFF3_E_GENE);
    bad += faulty("dangling_parent", joined({gene, tx, ex, ln("c1", "exon", "1", "9", "Parent=transcript:T")}), 4, DN_GFF3_E_PARENT);
    bad += faulty("dangling_grandparent", joined({tx, ex}), 2, DN_GFF3_E_PARENT);
    bad += faulty("no_nodes_at_all", ex + "\n", 1, DN_GFF3_E_PARENT);
    bad += faulty("parent_is_an_exon", joined({ln("c1", "exon", "1", "9", "ID=e1;gene=A"), ln("c1", "exon", "2", "9", "Parent=e1")}), 2, DN_GFF3_E_PARENT);
    bad += faulty("chain_9", chain(9), 1, DN_GFF3_E_DEPTH);
    bad += faulty("cycle_of_two", joined({ln("c1", "mRNA", "1", "9", "ID=a;Parent=b"), ln("c1", "mRNA", "1", "9", "ID=b;Parent=a"), own, ln("c1", "exon", "1", "9", "Parent=a")}),
                  4, DN_GFF3_E_DEPTH);
    bad += faulty("self_parent", joined({ln("c1", "mRNA", "1", "9", "ID=a;Parent=a"), ln("c1", "exon", "1", "9", "Parent=a")}), 2, DN_GFF3_E_DEPTH);
    {
        std::vector<std::string> lines = {gene, tx, ln("c1", "exon", "1", "9", "Parent=nobody")};
        for (int k = 0; k < 86; k++) lines.push_back(ex);
        lines.push_back("c1\tsrc\tgene\t1");
        bad += faulty("line_error_wins_over_link_error", joined(lines), 90, DN_GFF3_E_FIELDS);
    }
    bad += faulty("error_before_fasta", joined({gene, "oops", "##FASTA", ">c1"}), 2, DN_GFF3_E_FIELDS);

    // seeded damage: a byte replaced, often by one that matters to the rule, or a stretch cut out
    {
        std::vector<std::string> lines = {"##gff-version 3"};
        for (int g = 0; g < 6; g++) {
            const std::string k = std::to_string(g);
            lines.push_back(ln("c1", "gene", "1", "90", "ID=gene:G" + k + ";Name=NAME" + k + ";gene_id=G" + k));
            lines.push_back(ln("c1", "mRNA", "1", "90", "ID=transcript:T" + k + ";Parent=gene:G" + k));
            lines.push_back(ln("c1", "exon", "1", "9", "Parent=transcript:T" + k + ";Name=E" + k));
            lines.push_back(ln("c1", "CDS", "1", "9", "ID=cds" + k + ";Parent=transcript:T" + k));
            lines.push_back(g % 2 ? ln("c2", "exon", "1", "9", "ID=x" + k + ";gene=OWN" + k) : "###");
        }
        const std::string base = joined(lines);
        const std::string special("\t\n\r;=, #:0eEPI\0\xff", 17);
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
            if (t.empty()) continue;
            const Result r = scan(t, k % 2 ? 64 : 3);
            if (r.rc != DN_OK) { fprintf(stderr, "mutation %d: rc %d (%s)\n", k, r.rc, g_error.c_str()); bad++; break; }
            if (r.err_kind) errors++; else rows++;
        }
        printf("%-34s %lld with rows, %lld with an error: ok\n", "mutations", (long long) rows, (long long) errors);
    }
    return bad ? 1 : 0;
}

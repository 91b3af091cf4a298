"""
GPU tests of strand-specific counting end to end: prepare_inputs(..., stranded='reverse') on three small seeded samples and a
GTF, and on the GFF3 twin of the same annotation, against its twin runs -- the unstranded prepare_inputs on (A+, B+) and on
(A-, B-), per chromosome and in the stated gene order ('+' genes, then '-' genes) -- and `python -m degnorm_amd --stranded
reverse` on the same samples given as --sam-files, whose read_counts.csv and gene_exon_metadata.csv equal the function's;
`-w` on that directory runs, degnorm_amd.data_access writes a gene's two files from it, and stranded='no' writes tables and
matrices byte-identical to a call without the argument.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _flag_cases as fc                                        # noqa: E402
import _gtf_fixtures as gf                                      # noqa: E402
import _reads_fixtures as rf                                    # noqa: E402
import _strand_cases as sc                                      # noqa: E402
from degnorm_amd.pipeline import prepare_inputs                 # noqa: E402

pytestmark = pytest.mark.gpu

REFS = gf.PIPELINE_REFS
SAMPLES = gf.PIPELINE_SAMPLES
LAYOUTS = [rf.golden_layout(), rf.quiet_layout()]
STRAND_OF = {g: '+-'[k % 2] for _, _, genes in LAYOUTS for k, (g, _) in enumerate(genes)}      # genes alternate strands
KW = dict(minimax_coverage=1, verbose=False, pair='device')


def _write_annotation(path, strands=('+', '-')):
    """The genes of `strands` as a .gtf, or as a .gff3 whose exon lines name a transcript that names the gene."""
    gff3 = path.endswith('.gff3')
    with open(path, 'w') as f:
        if gff3:
            f.write('##gff-version 3\n')
        for chrom, _, genes in LAYOUTS:
            for g, exons in genes:
                s = STRAND_OF[g]
                if s not in strands:
                    continue
                a0, b0 = min(a for a, _ in exons), max(b for _, b in exons)
                if gff3:
                    f.write('{0}\ttest\tgene\t{1}\t{2}\t.\t{3}\t.\tID=gene:{4};Name={4}\n'.format(chrom, a0, b0, s, g))
                    f.write('{0}\ttest\tmRNA\t{1}\t{2}\t.\t{3}\t.\tID=tx:{4};Parent=gene:{4}\n'.format(chrom, a0, b0, s, g))
                    for a, b in exons:
                        f.write('{0}\ttest\texon\t{1}\t{2}\t.\t{3}\t.\tParent=tx:{4}\n'.format(chrom, a, b, s, g))
                else:
                    attr = 'gene_id "ID_{0}"; gene_name "{0}";'.format(g)
                    f.write('{0}\ttest\tgene\t{1}\t{2}\t.\t{3}\t.\t{4}\n'.format(chrom, a0, b0, s, attr))
                    for a, b in exons:
                        f.write('{0}\ttest\texon\t{1}\t{2}\t.\t{3}\t.\t{4}\n'.format(chrom, a, b, s, attr))


def _records(sample):
    rows = gf.pipeline_bam_rows(sample)
    rng = np.random.default_rng(40 + sample)
    return rows.assign(flag=rng.choice([0, fc.REVERSE], len(rows)), next_ref=-1, next_pos=-1, mapq=60)


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """The annotations, the three samples as .bam and .sam, their per-sense twins, and the twin runs; computed once."""
    d = tmp_path_factory.mktemp('strand_pipeline')
    w = {'dir': d, 'gtf': str(d / 'a.gtf'), 'gff3': str(d / 'a.gff3')}
    _write_annotation(w['gtf'])
    _write_annotation(w['gff3'])
    for s, tag in zip(sc.STRANDS, ('plus', 'minus')):
        w['gtf', s] = str(d / ('a_' + tag + '.gtf'))
        _write_annotation(w['gtf', s], strands=(s,))
    w['bam'], w['sam'] = [], []
    twins = {s: [] for s in sc.STRANDS}
    for k, name in enumerate(SAMPLES):
        os.makedirs(str(d / 'all'), exist_ok=True)
        p = str(d / 'all' / (name + '.bam'))
        written, _, _ = fc.write_bam(p, REFS, _records(k))
        w['bam'].append(p)
        sam = str(d / 'all' / (name + '.sam'))
        with open(sam, 'w') as f:
            f.write(fc.sam_header(REFS) + fc.sam_text(written, REFS))
        w['sam'].append(sam)
        sense = np.array([sc.sense_rule(int(fl), q, 'single', 'reverse') for fl, q in zip(written.flag, written.qname)], dtype=object)
        for s, tag in zip(sc.STRANDS, ('plus', 'minus')):
            os.makedirs(str(d / tag), exist_ok=True)
            q = str(d / tag / (name + '.bam'))
            fc.write_bam(q, REFS, written[sense == s])
            twins[s].append(q)
    for s, tag in zip(sc.STRANDS, ('plus', 'minus')):
        out = str(d / ('twin_out_' + tag))
        os.makedirs(out)
        w['twin', s] = prepare_inputs(twins[s], [b + '.bai' for b in twins[s]], w['gtf', s], out, **KW) + (out,)
    return w


def _stranded(w, annotation, out, **kw):
    os.makedirs(out, exist_ok=True)
    return prepare_inputs(w['bam'], [b + '.bai' for b in w['bam']], annotation, out, stranded='reverse', **dict(KW, **kw))


def _assert_equals_twins(w, got, out):
    cov, counts, genes_df, exon_df, sample_ids = got
    assert sample_ids == SAMPLES and 'strand' in genes_df.columns and 'strand' in exon_df.columns
    want_order = []
    for chrom in ('chr1', 'chr2'):
        for s in sc.STRANDS:
            t_cov, t_counts, t_genes, _, _, _ = w['twin', s]
            want_order += t_genes[t_genes.chr == chrom].gene.tolist()
    assert list(cov) == want_order == genes_df.gene.tolist() == counts.gene.tolist()
    assert len(want_order) >= 8 and {STRAND_OF[g] for g in want_order} == {'+', '-'}
    for s in sc.STRANDS:
        t_cov, t_counts, t_genes, _, _, _ = w['twin', s]
        for g in t_cov:
            assert STRAND_OF[g] == s and cov[g].dtype == t_cov[g].dtype and cov[g].tobytes() == t_cov[g].tobytes(), g
        mine = counts[counts.gene.isin(t_counts.gene)].reset_index(drop=True)
        pd.testing.assert_frame_equal(mine, t_counts.reset_index(drop=True))
    assert genes_df.strand.tolist() == [STRAND_OF[g] for g in genes_df.gene]
    # the unfiltered tables in the output directory: every stranded gene, each with the twin's counts; the strand column
    meta = pd.read_csv(os.path.join(out, 'gene_exon_metadata.csv'))
    assert list(meta.columns) == ['chr', 'start', 'end', 'gene', 'strand', 'gene_start', 'gene_end']
    assert meta.strand.tolist() == [STRAND_OF[g] for g in meta.gene]
    table = pd.read_csv(os.path.join(out, 'read_counts.csv'))
    for s in sc.STRANDS:
        t = pd.read_csv(os.path.join(w['twin', s][5], 'read_counts.csv'))
        pd.testing.assert_frame_equal(table[table.gene.isin(t.gene)].reset_index(drop=True), t)
    for chrom in ('chr1', 'chr2'):
        with open(os.path.join(out, chrom, 'coverage_matrices_{0}.pkl'.format(chrom)), 'rb') as f:
            mats = pickle.load(f)
        both = {}
        for s in sc.STRANDS:
            with open(os.path.join(w['twin', s][5], chrom, 'coverage_matrices_{0}.pkl'.format(chrom)), 'rb') as f:
                both.update(pickle.load(f))
        assert list(mats) == list(both) and all(mats[g].tobytes() == both[g].tobytes() for g in both)


@pytest.mark.parametrize('form', ['gtf', 'gff3'])
def test_stranded_prepare_inputs_equals_its_twin_runs(form, world, tmp_path):
    out = str(tmp_path / 'out')
    got = _stranded(world, world[form], out)
    _assert_equals_twins(world, got, out)
    # antisense reads are not counted: the unstranded run counts more
    plain_out = str(tmp_path / 'plain')
    os.makedirs(plain_out)
    plain = prepare_inputs(world['bam'], [b + '.bai' for b in world['bam']], world[form], plain_out, **KW)
    assert plain[1][SAMPLES].values.sum() > got[1][SAMPLES].values.sum() > 0


def test_device_settings_give_the_same_tables(world, tmp_path):
    got = _stranded(world, world['gtf'], str(tmp_path / 'out'), inflate='device', frame='device')
    _assert_equals_twins(world, got, str(tmp_path / 'out'))


def test_command_line_warm_start_and_data_access(world, tmp_path):
    out = str(tmp_path / 'fn')
    _stranded(world, world['gtf'], out)
    cli = str(tmp_path / 'cli')
    cmd = [sys.executable, '-m', 'degnorm_amd', '--stranded', 'reverse', '--device-pair', '--sam-files'] + world['sam'] + \
          ['-g', world['gtf'], '-o', cli, '--iter', '2', '--nmf-iter', '20', '--minimax-coverage', '1']
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'of sense +' in r.stdout and 'Rate of gene overlap' in r.stdout
    for name in ('read_counts.csv', 'gene_exon_metadata.csv'):
        with open(os.path.join(out, name), 'rb') as a, open(os.path.join(cli, name), 'rb') as b:
            assert a.read() == b.read(), name
    # -w on that directory runs
    warm = str(tmp_path / 'warm')
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd', '-w', cli, '-o', warm, '--iter', '2', '--nmf-iter', '20', '--minimax-coverage', '1'],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert os.path.isfile(os.path.join(warm, 'degradation_index_scores.csv'))
    # data_access on one gene of it writes its two files
    gene = pd.read_csv(os.path.join(cli, 'degradation_index_scores.csv')).gene.iloc[0]
    save = str(tmp_path / 'access')
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd.data_access', '-d', cli, '-g', gene, '-o', save],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    written = sorted(f for _, _, fs in os.walk(save) for f in fs)
    assert written == [gene.upper() + '_estimated_coverage.txt', gene.upper() + '_raw_coverage.txt'] or \
        written == [gene + '_estimated_coverage.txt', gene + '_raw_coverage.txt'], written


def test_stranded_no_is_the_call_without_the_argument(world, tmp_path):
    outs = []
    for k, kw in enumerate(({}, {'stranded': 'no'})):
        out = str(tmp_path / str(k))
        os.makedirs(out)
        prepare_inputs(world['bam'], [b + '.bai' for b in world['bam']], world['gtf'], out, **dict(KW, **kw))
        outs.append(out)
    files = sorted(os.path.relpath(os.path.join(r, f), outs[0]) for r, _, fs in os.walk(outs[0]) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(r, f), outs[1]) for r, _, fs in os.walk(outs[1]) for f in fs)
    assert 'read_counts.csv' in files and 'gene_exon_metadata.csv' in files and len(files) >= 4
    for f in files:
        with open(os.path.join(outs[0], f), 'rb') as a, open(os.path.join(outs[1], f), 'rb') as b:
            assert a.read() == b.read(), f
    assert 'strand' not in pd.read_csv(os.path.join(outs[0], 'gene_exon_metadata.csv')).columns

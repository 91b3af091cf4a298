"""
GPU tests of strand-specific counting from .bam files: NativeBamReadsProcessor(..., stranded='forward' | 'reverse') against
its twin, the unstranded processor on (A+, B+) and on (A-, B-) -- the guarantee of include/degnorm_amd.h, "Strand-specific
counting".  A^s is the genes of strand s, B^s a .bam file of the records whose sense is s (the restatement of
tests/_strand_cases.py decides), in file order.  Every comparison is exact: the read-count table, the overlap pickle and
both CSR rows.

About 3 000 seeded reads (or 1 500 pairs) over a seeded annotation of 60 genes on both strands, strand bits random:
single-end, paired by FLAG, paired by the name rule (g<k>.1 / g<k>.2; the twin runs under pair='device'), windows of 20 kB,
both inflate settings with both frame settings; the skip-if-present rule on the four file names; load_chromosome_reads'
`sense` column.
"""
import os
import pickle
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _flag_cases as fc                                        # noqa: E402
import _reads_fixtures as rf                                    # noqa: E402
import _reads_oracle as ro                                      # noqa: E402
import _strand_cases as sc                                      # noqa: E402
from degnorm_amd import bam                                     # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure   # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 21
KINDS = ('single', 'flag', 'name')
OPTIONS = {'single': {}, 'flag': {'pairing': 'flag'}, 'name': {'pairing': 'name'}}
CHROM = 'chrS'


def _records(kind, layout):
    """The records of one kind of file, unsorted: DataFrame(ref, pos, qname, cigar, flag, next_ref, next_pos, mapq)."""
    rng = np.random.default_rng([SEED, KINDS.index(kind)])
    if kind == 'single':
        src = rf.synth_reads(SEED, layout, 3000, skip=())
        return src.assign(ref=0, flag=rng.choice([0, fc.REVERSE], len(src)), next_ref=-1, next_pos=-1, mapq=60)
    flagged, twin = fc.flag_style(rf.synth_pairs(SEED + 1, layout, 1500, skip=()), seed=SEED)
    # under the name rule only the name tells the mates apart: FLAG keeps its strand bit alone
    return flagged if kind == 'flag' else twin.assign(flag=twin.flag & fc.REVERSE)


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """
    The annotation, and per kind of file: the .bam, its records in file order, and per protocol the senses, the two twin
    files B+ and B- and the twin's outputs on (A+, B+) and (A-, B-).  Computed once and not changed by any test.
    """
    from test_gpu_bam import _run
    root = tmp_path_factory.mktemp('strand_bam')
    chrom, chrom_len, genes, strand_of = sc.two_strand_layout(SEED)
    gene_df, exon_df = rf.tables(chrom, genes)
    gene_df = gene_df.assign(strand=[strand_of[g] for g in gene_df.gene])
    exon_df = exon_df.assign(strand=[strand_of[g] for g in exon_df.gene])
    parts = sc.split_tables(gene_df, exon_df, strand_of)
    refs = [(chrom, chrom_len), ('chrO', chrom_len)]
    w = {'chrom_len': chrom_len, 'genes': genes, 'strand_of': strand_of, 'gene_df': gene_df, 'exon_df': exon_df, 'parts': parts,
         'ov': get_gene_overlap_structure(gene_df), 'root': root}
    for kind in KINDS:
        path = str(root / (kind + '.bam'))
        written, _, _ = fc.write_bam(path, refs, _records(kind, (chrom, chrom_len, genes)), straddle=True)
        k = {'path': path, 'written': written}
        for protocol in sc.PROTOCOLS:
            sense = np.array([sc.sense_rule(int(f), q, kind, protocol) for f, q in zip(written.flag, written.qname)], dtype=object)
            twin = {}
            for s in sc.STRANDS:
                p = str(root / '{0}_{1}_{2}.bam'.format(kind, protocol, 'plus' if s == '+' else 'minus'))
                fc.write_bam(p, refs, written[sense == s], straddle=True)
                ov, g, e = parts[s]
                twin[s] = _run(p, CHROM, ov, g.drop(columns='strand'), e.drop(columns='strand'), root / ('twin_' + kind + protocol + s),
                               pair='device', **OPTIONS[kind])[1]
            k[protocol] = {'sense': sense, 'twin': twin}
        w[kind] = k
    return w


def _stranded_run(w, kind, protocol, out, **kw):
    proc = bam.NativeBamReadsProcessor(w[kind]['path'], w[kind]['path'] + '.bai', output_dir=str(out), verbose=False, stranded=protocol,
                                       **dict(OPTIONS[kind], **kw))
    os.makedirs(proc.save_dir, exist_ok=True)
    proc.chromosome_coverage_read_counts(w['ov'], w['gene_df'], w['exon_df'], CHROM)
    return proc


def _assert_twin(w, kind, protocol, proc):
    from scipy import sparse
    cov_files, ol_file, count_file = proc._files(CHROM)
    twin = w[kind][protocol]['twin']
    tag = proc.sample_id + '_' + CHROM
    assert sorted(os.listdir(proc.save_dir)) == sorted(os.path.basename(f) for f in [ol_file, count_file] + [
        cov_files[s] for s in sc.STRANDS if twin[s][0] is not None])
    assert [os.path.basename(cov_files[s]) for s in sc.STRANDS] == ['chrom_coverage_' + tag + '_plus.npz', 'chrom_coverage_' + tag + '_minus.npz']
    assert not os.path.exists(os.path.join(proc.save_dir, 'chrom_coverage_' + tag + '.npz'))
    # read counts: all genes, in chrom_gene_df order; each the twin's of its strand
    cnt = pd.read_csv(count_file)
    assert list(cnt.columns) == ['gene', proc.sample_id] and cnt.gene.tolist() == w['gene_df'].gene.tolist()
    want = {}
    for s in sc.STRANDS:
        t = twin[s][2]
        assert t.gene.tolist() == w['parts'][s][1].gene.tolist()
        want.update(zip(t.gene, t.iloc[:, 1].astype(int)))
    assert dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int))) == want
    # the overlap pickle: the overlap genes of '+', then those of '-'
    with open(ol_file, 'rb') as f:
        ol = pickle.load(f)
    assert list(ol) == list(twin['+'][1]) + list(twin['-'][1]) and len(twin['+'][1]) > 1 and len(twin['-'][1]) > 1
    for s in sc.STRANDS:
        for g, v in twin[s][1].items():
            assert ol[g].dtype == v.dtype and ol[g].tobytes() == v.tobytes(), g
    # both CSR rows
    for s in sc.STRANDS:
        assert twin[s][0] is not None, s                        # the case reaches the isolated stage on both strands
        csr = sparse.load_npz(cov_files[s])
        assert csr.shape == twin[s][0].shape and csr.dtype == twin[s][0].dtype
        assert csr.indices.tobytes() == twin[s][0].indices.tobytes() and csr.data.tobytes() == twin[s][0].data.tobytes(), s
    return want


def test_the_case_has_what_it_is_for(world):
    w = world
    assert len(w['gene_df']) == 60
    for s in sc.STRANDS:
        ov = w['parts'][s][0]
        assert len(ov['overlap_genes']) >= 1 and len(ov['isolated_genes']) >= 5, s
    assert len(sc.shared_exon_pairs(w['genes'], w['strand_of'])) >= 3
    # single-end: the restatement's counts by strand against its unstranded counts
    reads = w['single']['written']
    reads = reads[reads.ref == 0]
    plain = ro.restate(reads, w['chrom_len'], w['ov'], w['gene_df'], w['exon_df'], False)[2]
    sense = w['single']['forward']['sense'][(w['single']['written'].ref == 0).values]
    stranded = {}
    for s in sc.STRANDS:
        stranded.update(sc.expected(reads, sense, w['chrom_len'], w['parts'], s, False)[2])
    differ = sum(stranded[g] != plain[g] for g in plain)
    print('genes whose stranded count differs from the unstranded one:', differ, 'of', len(plain))
    assert 4 * differ >= len(plain)
    for kind in ('flag', 'name'):
        written = w[kind]['written']
        key = written.qname if kind == 'flag' else written.qname.str[:-2]
        bad = sc.disagreeing_pairs(pd.DataFrame({'qname_unpaired': key.values}), w[kind]['forward']['sense'])
        print(kind, 'pairs whose mates disagree:', len(bad))
        assert len(bad) >= 20


@pytest.mark.parametrize('protocol', sc.PROTOCOLS)
@pytest.mark.parametrize('kind', KINDS)
def test_stranded_run_equals_its_twin(kind, protocol, world, tmp_path):
    proc = _stranded_run(world, kind, protocol, tmp_path)
    assert proc.paired == (kind != 'single') and proc.pairing_rule == ('flag' if kind == 'flag' else 'name')
    counts = _assert_twin(world, kind, protocol, proc)
    assert sum(counts.values()) > 150
    if kind != 'single':
        assert proc.timing['pair_device_ms'] > 0.0


def test_forward_and_reverse_swap_the_rows(world, tmp_path):
    w = world
    for kind in KINDS:
        f, r = w[kind]['forward']['sense'], w[kind]['reverse']['sense']
        assert (f != r).all() and set(f) == {'+', '-'}
    a = _assert_twin(w, 'single', 'forward', _stranded_run(w, 'single', 'forward', tmp_path / 'f'))
    b = _assert_twin(w, 'single', 'reverse', _stranded_run(w, 'single', 'reverse', tmp_path / 'r'))
    assert a != b


@pytest.mark.parametrize('kind', ['single', 'flag'])
def test_windows_of_20_kb(kind, world, tmp_path):
    proc = _stranded_run(world, kind, 'reverse', tmp_path, window_bytes=20000)
    _assert_twin(world, kind, 'reverse', proc)


@pytest.mark.parametrize('frame', ['host', 'device'])
@pytest.mark.parametrize('inflate', ['host', 'device'])
def test_inflate_and_frame_settings(inflate, frame, world, tmp_path):
    for kind in ('name', 'single'):
        proc = _stranded_run(world, kind, 'reverse', tmp_path / kind, inflate=inflate, frame=frame, window_bytes=50000)
        _assert_twin(world, kind, 'reverse', proc)


def test_skip_if_present_asks_for_the_stranded_names(world, tmp_path):
    w = world
    proc = _stranded_run(w, 'single', 'forward', tmp_path)
    cov_files, ol_file, count_file = proc._files(CHROM)
    files = [cov_files['+'], cov_files['-'], ol_file, count_file]
    assert all(os.path.isfile(f) for f in files)

    def rerun():
        before = {f: os.stat(f).st_mtime_ns for f in files if os.path.isfile(f)}
        calls = []
        proc.device_rows, keep = (lambda chrom: calls.append(chrom) or keep(chrom)), proc.device_rows
        try:
            proc.chromosome_coverage_read_counts(w['ov'], w['gene_df'], w['exon_df'], CHROM)
        finally:
            proc.device_rows = keep
        return bool(calls), before

    ran, _ = rerun()
    assert not ran                                              # all four present: nothing is computed
    # the unstranded name does not stand in for a stranded one
    unstranded = os.path.join(proc.save_dir, 'chrom_coverage_' + proc.sample_id + '_' + CHROM + '.npz')
    for f in files:
        os.rename(f, f + '.away')
        if f in cov_files.values():
            with open(unstranded, 'wb') as g:
                g.write(b'not read')
        ran, _ = rerun()
        assert ran and os.path.isfile(f), f
        os.remove(f + '.away')
        if os.path.exists(unstranded):
            with open(unstranded, 'rb') as g:
                assert g.read() == b'not read'
            os.remove(unstranded)
    _assert_twin(w, 'single', 'forward', proc)


@pytest.mark.parametrize('kind', KINDS)
def test_load_chromosome_reads_has_the_sense_column(kind, world, tmp_path):
    w = world
    for protocol in sc.PROTOCOLS:
        proc = bam.NativeBamReadsProcessor(w[kind]['path'], w[kind]['path'] + '.bai', output_dir=str(tmp_path), verbose=False,
                                           stranded=protocol, **OPTIONS[kind])
        df = proc.load_chromosome_reads(CHROM)
        assert 'sense' in df.columns and len(df) > 1000
        want = {q: s for q, s, ref in zip(w[kind]['written'].qname, w[kind][protocol]['sense'], w[kind]['written'].ref) if ref == 0}
        if kind == 'flag':                                      # both mates carry one name: tell them by FLAG
            assert df.sense.tolist() == [sc.sense_rule(int(f), q, kind, protocol) for f, q in zip(df.flag, df.qname)]
        else:
            assert df.sense.tolist() == [want[q] for q in df.qname]
        assert set(df.sense) == {'+', '-'}
    plain = bam.NativeBamReadsProcessor(w[kind]['path'], w[kind]['path'] + '.bai', output_dir=str(tmp_path), verbose=False, **OPTIONS[kind])
    assert 'sense' not in plain.load_chromosome_reads(CHROM).columns

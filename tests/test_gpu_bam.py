"""
GPU tests of the native BAM reader (degnorm_amd.bam.NativeBamReadsProcessor, csrc/dn_reads.hip): the reference's goldens
read from BAM files, paired reads against the in-memory path on the DataFrame the reference's load_chromosome_reads rules
give, the read filters and errors, the binary CIGAR parser on the fuzz goldens, small windows, run-to-run identity and a
1 M-read scale case.
"""
import os
import pickle
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_reads import _case, _check, _expect              # noqa: E402
from degnorm_amd import bam                                    # noqa: E402
from degnorm_amd import reads as dr                            # noqa: E402
from degnorm_amd.gene_processing import get_gene_overlap_structure   # noqa: E402

pytestmark = pytest.mark.gpu


def _files(proc, chrom):
    from scipy import sparse
    f_csr, f_ol, f_cnt = proc._files(chrom)
    csr = sparse.load_npz(f_csr) if os.path.isfile(f_csr) else None
    ol = None
    if os.path.isfile(f_ol):
        with open(f_ol, 'rb') as f:
            ol = pickle.load(f)
    cnt = pd.read_csv(f_cnt)
    return csr, ol, cnt


def _run(path, chrom, ov, gene_df, exon_df, out, **kw):
    proc = bam.NativeBamReadsProcessor(path, path + '.bai', output_dir=str(out), verbose=False, **kw)
    os.makedirs(proc.save_dir, exist_ok=True)
    proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
    return proc, _files(proc, chrom)


def _same(a, b):
    (ca, oa, na), (cb, ob, nb) = a, b
    assert (ca is None) == (cb is None)
    if ca is not None:
        assert ca.indices.tobytes() == cb.indices.tobytes() and ca.data.tobytes() == cb.data.tobytes()
    assert (oa is None) == (ob is None)
    if oa is not None:
        assert list(oa) == list(ob) and all(oa[g].tobytes() == ob[g].tobytes() for g in oa)
    pd.testing.assert_frame_equal(na, nb)


def expected_frame(reads, tid, unique_alignment, paired):
    """The reference's load_chromosome_reads on the written records (file order): its filters, then reads_frame."""
    r = reads[reads.ref == tid]
    if unique_alignment and 'nh' in r:
        r = r[~r.nh.apply(lambda v: v is not None and v == v and v > 1)]
    if paired:
        r = r[r.next_ref != -1]
    cig = [c if isinstance(c, str) and c else None for c in r.cigar]
    return dr.reads_frame(list(zip(r.qname.astype(str), r.pos.astype(int), cig)), paired)


@pytest.mark.parametrize('key', ['se', 'qi'])
@pytest.mark.parametrize('straddle', [False, True])
def test_bam_files_match_reference_golden(key, straddle, tmp_path):
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    assert not paired
    df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': ['r{0}'.format(i) for i in range(len(reads))],
                       'cigar': reads.cigar.values, 'nh': 1, 'nh_type': 'C'})
    p = str(tmp_path / (key + '.bam'))
    bf.write_bam(p, [('c', chrom_len)], df, straddle=straddle)
    proc, (csr, ol, cnt) = _run(p, 'c', ov, gene_df, exon_df, tmp_path / 'out')
    assert not proc.paired and list(cnt.columns) == ['gene', key]
    _check(csr, ol, dict(zip(cnt.gene, cnt[key].astype(int))), _expect(z, key))
    assert cnt.gene.tolist() == gene_df.gene.tolist()


def test_paired_equals_in_memory_path(tmp_path):
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, 'pe')
    assert paired
    pair = z['pe_pair']
    mate = np.zeros(len(pair), dtype=np.int64)
    mate[1:] = (pair[1:] == pair[:-1]).astype(np.int64)
    df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': ['{0}.{1}'.format(a, b + 1) for a, b in zip(pair, mate)],
                       'cigar': reads.cigar.values, 'next_ref': 0})
    p = str(tmp_path / 'pe.bam')
    written, _, _ = bf.write_bam(p, [('c', chrom_len)], df, straddle=True)
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / 'out'), verbose=False)
    assert proc.paired
    expect = expected_frame(written, 0, True, True)
    pd.testing.assert_frame_equal(proc.load_chromosome_reads('c'), expect)
    csr_e, ol_e, counts_e = dr.chromosome_coverage_read_counts_df(expect, chrom_len, ov, gene_df, exon_df, True)
    os.makedirs(proc.save_dir)
    proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, 'c')
    csr, ol, cnt = _files(proc, 'c')
    assert sum(counts_e.values()) > 100
    assert dict(zip(cnt.gene, cnt.pe.astype(int))) == counts_e
    assert (csr is None) == (csr_e is None)
    if csr is not None:
        np.testing.assert_array_equal(csr.indices, csr_e.indices)
        np.testing.assert_array_equal(csr.data, csr_e.data)
    assert list(ol) == list(ol_e) and all(np.array_equal(ol[g], ol_e[g]) for g in ol_e)


def _layout_case(seed, n, paired):
    chrom, chrom_len, genes = rf.golden_layout()
    gene_df, exon_df = rf.tables(chrom, genes)
    ov = get_gene_overlap_structure(gene_df)
    src = rf.synth_pairs(seed, (chrom, chrom_len, genes), n) if paired else rf.synth_reads(seed, (chrom, chrom_len, genes), n)
    return chrom, chrom_len, gene_df, exon_df, ov, src


@pytest.mark.parametrize('paired', [False, True])
@pytest.mark.parametrize('unique', [True, False])
def test_filters_match_reference_rules(paired, unique, tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(7, 1500, paired)
    rng = np.random.default_rng(3)
    n = len(src)
    nh = rng.choice([1, 2, 3, 1, None], n).tolist()
    nh_type = rng.choice(['C', 'S', 'i', 'c', 's', 'I'], n).tolist()
    df = pd.DataFrame({'ref': 1, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values,
                       'nh': nh, 'nh_type': nh_type, 'next_ref': np.where(rng.random(n) < 0.1, -1, 1)})
    # reads of other chromosomes (before and after) must never leak in
    other = df.sample(400, random_state=1).assign(ref=0)
    other2 = df.sample(300, random_state=2).assign(ref=2, qname=lambda d: 'z' + d.qname)
    refs = [('chrA', chrom_len), (chrom, chrom_len), ('chrZ', chrom_len)]
    p = str(tmp_path / 'f.bam')
    written, _, _ = bf.write_bam(p, refs, pd.concat([df, other, other2]), straddle=True)
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / 'out'), unique_alignment=unique,
                                       chroms=[chrom], verbose=False)
    proc.paired = paired                                            # the filters under test, whatever the names say
    expect = expected_frame(written, 1, unique, paired)
    got = proc.load_chromosome_reads(chrom)
    pd.testing.assert_frame_equal(got, expect)
    assert len(expect) < (written.ref == 1).sum() or not unique
    csr_e, ol_e, counts_e = dr.chromosome_coverage_read_counts_df(expect, chrom_len, ov, gene_df, exon_df, paired)
    os.makedirs(proc.save_dir)
    proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
    csr, ol, cnt = _files(proc, chrom)
    assert dict(zip(cnt.gene, cnt.iloc[:, 1].astype(int))) == counts_e
    assert (csr is None) == (csr_e is None)
    if csr is not None:
        assert csr.indices.tobytes() == csr_e.indices.tobytes() and csr.data.tobytes() == csr_e.data.tobytes()
    assert all(np.array_equal(ol[g], ol_e[g]) for g in ol_e)


def test_errors(tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(9, 200, False)
    base = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values})

    def proc_for(df, name, **kw):
        p = str(tmp_path / (name + '.bam'))
        bf.write_bam(p, [(chrom, chrom_len)], df)
        return bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / name), verbose=False, **kw)

    # a kept row without CIGAR (a placed unmapped mate): ValueError naming the read; dropped by NH it is harmless
    d = base.copy()
    d.loc[5, 'cigar'] = None
    d.loc[5, 'qname'] = 'lonely'
    p = proc_for(d.assign(flag=np.where(d.index == 5, 4, 0)), 'nocig')
    assert p.load_chromosome_reads(chrom).cigar.isna().sum() == 1
    os.makedirs(p.save_dir)
    with pytest.raises(ValueError, match='lonely'):
        p.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
    d['nh'] = [None] * len(d)
    d.loc[5, 'nh'] = 4
    p = proc_for(d, 'nocig_dropped')
    os.makedirs(p.save_dir)
    p.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
    # NH of a non-integer type
    d = base.assign(nh=2, nh_type=['Z' if i == 7 else 'C' for i in range(len(base))])
    with pytest.raises(ValueError, match='NH'):
        proc_for(d, 'nhz').load_chromosome_reads(chrom)
    assert len(proc_for(d, 'nhz_off', unique_alignment=False).load_chromosome_reads(chrom)) == len(d)
    # a CIGAR left in the CG tag's placeholder form is not supported
    d = base.copy()
    d.loc[3, 'cigar'] = '0S100N'
    pr = proc_for(d, 'cg')
    from degnorm_amd import _lib
    # the placeholder alone (no CG tag) is an ordinary CIGAR; with op codes above 8 it is refused
    assert len(pr.load_chromosome_reads(chrom)) == len(d)
    rows = bam.DeviceRows(0, True, False)
    rec = bytearray(bf.encode_records(base.iloc[:3])[0])
    off = np.array([0], dtype=np.int64)
    l_name = rec[12]
    rec[36 + l_name:40 + l_name] = (50 << 4 | 9).to_bytes(4, 'little')
    with pytest.raises(_lib.DegnormAmdError, match='op code'):
        rows.append(bytes(rec), off)
    rows.close()


def test_chromosome_without_reads(tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(4, 300, False)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values})
    p = str(tmp_path / 'e.bam')
    bf.write_bam(p, [('other', chrom_len), (chrom, chrom_len)], df)
    proc, (csr, ol, cnt) = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'out')
    assert csr is None and not os.path.isfile(proc._files(chrom)[0])
    assert (cnt.iloc[:, 1] == 0).all() and len(cnt) == len(gene_df)
    assert all((v == 0).all() for v in ol.values())
    assert len(proc.load_chromosome_reads(chrom)) == 0


def test_binary_cigar_parser_matches_reference_fuzz():
    from degnorm_amd import _lib
    import ctypes
    z = golden('reads')
    off, buf = z['fz_cig_off'], z['fz_cig'].tobytes()
    packed = [bf._binary_cigar(buf[off[i]:off[i + 1]].decode()) for i in range(len(off) - 1)]
    ops = np.frombuffer(b''.join(c for c, _, _ in packed), dtype='<u4').astype(np.uint32)
    op_off = np.zeros(len(packed) + 1, dtype=np.int64)
    op_off[1:] = np.cumsum([k for _, k, _ in packed])
    n, max_seg = len(packed), 16
    pos = np.ascontiguousarray(z['fz_pos'], dtype=np.int64)
    nseg = np.zeros(n, np.int32)
    bounds = np.zeros(n * 2 * max_seg, np.int64)
    end_pos = np.zeros(n, np.int64)
    P = ctypes.POINTER
    rc = _lib.load().dn_bam_cigar_bounds(0, n, pos.ctypes.data_as(P(ctypes.c_int64)), op_off.ctypes.data_as(P(ctypes.c_int64)),
                                         ops.ctypes.data_as(P(ctypes.c_uint32)), max_seg, nseg.ctypes.data_as(P(ctypes.c_int32)),
                                         bounds.ctypes.data_as(P(ctypes.c_int64)), end_pos.ctypes.data_as(P(ctypes.c_int64)))
    assert rc == 0
    np.testing.assert_array_equal(nseg, z['fz_nseg'])
    b = bounds.reshape(n, 2 * max_seg)
    flat = np.concatenate([b[r, :2 * k] for r, k in enumerate(nseg.tolist())])
    np.testing.assert_array_equal(flat, z['fz_bounds'])
    np.testing.assert_array_equal(end_pos, z['fz_end_pos'])


def test_small_windows_and_run_to_run(tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(12, 3000, True)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values, 'next_ref': 0})
    p = str(tmp_path / 'w.bam')
    bf.write_bam(p, [(chrom, chrom_len)], df, straddle=True)
    outs = []
    for k, (wb, jobs) in enumerate([(256 << 20, 1), (4096, 1), (4096, 3), (256 << 20, 2)]):
        proc, got = _run(p, chrom, ov, gene_df, exon_df, tmp_path / 'o{0}'.format(k), window_bytes=4096 if wb == 4096 else wb,
                         n_jobs=jobs)
        assert proc.paired
        outs.append(got)
    for o in outs[1:]:
        _same(outs[0], o)


def test_scale_single_end_equals_in_memory(tmp_path):
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case(n_reads=1_000_000)
    df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
    p = str(tmp_path / 'big.bam')
    bf.write_bam(p, [('chrS', chrom_len)], df)
    csr_e, ol_e, counts_e = dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, False)
    proc, (csr, ol, cnt) = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / 'out', n_jobs=4)
    assert dict(zip(cnt.gene, cnt.big.astype(int))) == counts_e and sum(counts_e.values()) > 500000
    assert csr.indices.tobytes() == csr_e.indices.tobytes() and csr.data.tobytes() == csr_e.data.tobytes()
    assert sorted(ol) == sorted(ol_e) and all(np.array_equal(ol[g], ol_e[g]) for g in ol_e)

"""
GPU tests of the BGZF inflate kernel (csrc/dn_inflate.hip) and of NativeBamReadsProcessor(inflate='device'): every valid case
of tests/_inflate_cases.py in one launch against zlib, corrupt blocks (each first refused by the host build of the same
source) among valid ones, and the device-inflate reader against the host-inflate reader on the goldens, small windows,
trimmed index ranges, the filter cases, the 1 M-read scale case, a damaged file and the BAM + GTF pipeline.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _inflate_cases as ic                                    # noqa: E402
import _reads_fixtures as rf                                   # noqa: E402
from conftest import golden                                    # noqa: E402
from test_gpu_reads import _case                               # noqa: E402
from test_gpu_bam import _files, _layout_case, _run, _same     # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

pytestmark = pytest.mark.gpu

_VALID_PASSED = []                                             # set by the valid-input test: the corrupt batch runs only after it


@pytest.fixture(scope='module')
def cases():
    return ic.valid_cases()


def test_all_valid_cases_in_one_launch(cases):
    blocks = ic.blocks_of(cases)
    got = bam.inflate_blocks(blocks, device=0)
    assert len(got) == len(cases)
    for (name, data, _), g in zip(cases, got):
        assert g == data, name
    order = np.random.default_rng(5).permutation(len(cases))
    got = bam.inflate_blocks([blocks[k] for k in order] * 3, device=0)
    for j, g in enumerate(got):
        assert g == cases[order[j % len(cases)]][1], cases[order[j % len(cases)]][0]
    _VALID_PASSED.append(True)


def test_corrupt_blocks_among_valid_ones(cases):
    """Error paths the host build has already walked: 32 refused mutations, spread over the kinds, between valid blocks."""
    import ctypes
    from degnorm_amd import _lib
    assert _VALID_PASSED, 'no corrupt block goes to the device before test_all_valid_cases_in_one_launch has passed in this run'
    refused = {}
    for kind, payload, isize in ic.mutations():
        if len(refused.setdefault(kind, [])) < 5:
            rc, status, _ = ic.host_inflate(payload, isize)
            if rc == 0 and status != 0:
                refused[kind].append((payload, isize, status))
    bad = [m for kind in sorted(refused) for m in refused[kind]][:32]
    assert len(bad) == 32
    valid = [(p, len(d), d) for _, d, p in cases]
    blocks, expect = [], []
    for k, (p, n, d) in enumerate(valid):
        blocks.append((p, n))
        expect.append((0, d))
        if k < len(bad):
            blocks.append(bad[k][:2])
            expect.append((bad[k][2], None))
    comp = np.frombuffer(b''.join(p for p, _ in blocks), np.uint8)
    pay_len = np.array([len(p) for p, _ in blocks], np.int32)
    pay_off = np.zeros(len(blocks), np.int64)
    pay_off[1:] = np.cumsum(pay_len[:-1])
    out_off = np.zeros(len(blocks) + 1, np.int64)
    out_off[1:] = np.cumsum([n for _, n in blocks])
    out, status = np.zeros(int(out_off[-1]) + 1, np.uint8), np.full(len(blocks), -9, np.int32)
    P, c = ctypes.POINTER, ctypes
    rc = _lib.load().dn_bgzf_inflate(0, comp.ctypes.data_as(P(c.c_uint8)), len(comp), len(blocks), pay_off.ctypes.data_as(P(c.c_int64)),
                                     pay_len.ctypes.data_as(P(c.c_int32)), out_off.ctypes.data_as(P(c.c_int64)),
                                     out.ctypes.data_as(P(c.c_uint8)), status.ctypes.data_as(P(c.c_int32)), None, None)
    assert rc == 0
    for b, (st, d) in enumerate(expect):
        assert status[b] == st, (b, status[b], st)              # the device reports what the host build reported
        if d is not None:
            assert out[out_off[b]:out_off[b + 1]].tobytes() == d, b
    with pytest.raises(ValueError, match='BGZF block 1 does not inflate'):
        bam.inflate_blocks([ic.bgzf(*blocks[0]), ic.bgzf(*blocks[1])], device=0)
    # the next call on the same process works
    assert bam.inflate_blocks(ic.blocks_of(cases[:8]), device=0) == [d for _, d, _ in cases[:8]]


def _both(path, chrom, ov, gene_df, exon_df, out, **kw):
    """Host-inflate and device-inflate runs of one file: output files and load_chromosome_reads frames must be identical."""
    res = {}
    for mode in ('host', 'device'):
        proc, files = _run(path, chrom, ov, gene_df, exon_df, os.path.join(str(out), mode), inflate=mode, **kw)
        res[mode] = (proc, files, proc.load_chromosome_reads(chrom))
    _same(res['host'][1], res['device'][1])
    pd.testing.assert_frame_equal(res['host'][2], res['device'][2])
    assert res['device'][0].timing['inflate_device_ms'] > 0 and 'inflate_device_ms' not in res['host'][0].timing
    return res


@pytest.mark.parametrize('level', [1, 6])
@pytest.mark.parametrize('straddle', [False, True])
@pytest.mark.parametrize('key', ['se', 'qi', 'pe'])
def test_reader_equals_host_inflate_on_goldens(key, straddle, level, tmp_path):
    z = golden('reads')
    reads, chrom_len, ov, gene_df, exon_df, paired = _case(z, key)
    if paired:
        pair = z['pe_pair']
        mate = np.zeros(len(pair), dtype=np.int64)
        mate[1:] = (pair[1:] == pair[:-1]).astype(np.int64)
        df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': ['{0}.{1}'.format(a, b + 1) for a, b in zip(pair, mate)],
                           'cigar': reads.cigar.values, 'next_ref': 0})
    else:
        df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': ['r{0}'.format(i) for i in range(len(reads))],
                           'cigar': reads.cigar.values, 'nh': 1, 'nh_type': 'C'})
    p = str(tmp_path / (key + '.bam'))
    bf.write_bam(p, [('c', chrom_len)], df, straddle=straddle, level=level)
    res = _both(p, 'c', ov, gene_df, exon_df, tmp_path)
    assert res['device'][0].paired == paired and len(res['device'][2]) > 100


@pytest.mark.parametrize('window_bytes', [1, 70000, None])
def test_windows_carry_and_trims(window_bytes, tmp_path):
    """Three references, the middle one read: its index range starts and ends inside blocks it shares with its neighbours."""
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(21, 4000, True)
    df = pd.DataFrame({'ref': 1, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values, 'next_ref': 1})
    before = df.sample(700, random_state=1).assign(ref=0)
    after = df.sample(600, random_state=2).assign(ref=2, qname=lambda d: 'z' + d.qname)
    p = str(tmp_path / 'three.bam')
    bf.write_bam(p, [('chrA', chrom_len), (chrom, chrom_len), ('chrZ', chrom_len)], pd.concat([df, before, after]), straddle=True, level=6)
    ref = bam.read_bai(p + '.bai')[0][1]
    vbeg, vend = bam.reference_range(ref)
    assert vbeg & 0xffff and vend & 0xffff and (vend >> 16) > (vbeg >> 16)           # head and tail trims both non-zero
    kw = {} if window_bytes is None else {'window_bytes': window_bytes}
    res = _both(p, chrom, ov, gene_df, exon_df, tmp_path, chroms=[chrom], **kw)
    assert len(res['device'][2]) > 1000


@pytest.mark.parametrize('paired', [False, True])
@pytest.mark.parametrize('unique', [True, False])
def test_filter_cases(paired, unique, tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(7, 1500, paired)
    rng = np.random.default_rng(3)
    n = len(src)
    df = pd.DataFrame({'ref': 1, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values,
                       'nh': rng.choice([1, 2, 3, 1, None], n).tolist(), 'nh_type': rng.choice(['C', 'S', 'i', 'c', 's', 'I'], n).tolist(),
                       'next_ref': np.where(rng.random(n) < 0.1, -1, 1)})
    other = df.sample(400, random_state=1).assign(ref=0)
    other2 = df.sample(300, random_state=2).assign(ref=2, qname=lambda d: 'z' + d.qname)
    p = str(tmp_path / 'f.bam')
    bf.write_bam(p, [('chrA', chrom_len), (chrom, chrom_len), ('chrZ', chrom_len)], pd.concat([df, other, other2]), straddle=True)
    frames = {}
    for mode in ('host', 'device'):
        proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / mode), unique_alignment=unique, chroms=[chrom],
                                           verbose=False, inflate=mode)
        proc.paired = paired
        frames[mode] = proc.load_chromosome_reads(chrom)
        os.makedirs(proc.save_dir)
        proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
        frames[mode + '_files'] = _files(proc, chrom)
    pd.testing.assert_frame_equal(frames['host'], frames['device'])
    _same(frames['host_files'], frames['device_files'])
    assert 0 < len(frames['device']) <= n


def test_scale_case_equals_host_and_repeats(tmp_path):
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case(n_reads=1_000_000)
    df = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
    p = str(tmp_path / 'big.bam')
    bf.write_bam(p, [('chrS', chrom_len)], df)
    _, host = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / 'host', n_jobs=4)
    _, dev1 = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / 'dev1', inflate='device')
    _, dev2 = _run(p, 'chrS', ov, gene_df, exon_df, tmp_path / 'dev2', inflate='device', window_bytes=32 << 20)
    assert int(host[2].iloc[:, 1].sum()) > 500000
    _same(host, dev1)
    _same(dev1, dev2)


def test_damaged_block_names_file_and_offset(tmp_path):
    chrom, chrom_len, gene_df, exon_df, ov, src = _layout_case(31, 3000, False)
    df = pd.DataFrame({'ref': 0, 'pos': src.pos.values, 'qname': src.qname.values, 'cigar': src.cigar.values})
    good = df.assign(qname=lambda d: 'g' + d.qname)             # chrG comes first: the constructor's look at the first reads stays clean
    p = str(tmp_path / 'd.bam')
    bf.write_bam(p, [('chrG', chrom_len), (chrom, chrom_len)], pd.concat([df.assign(ref=1), good]), block_size=20000, level=6)
    offs, sizes, _ = bam.bgzf_blocks(p)
    vbeg, vend = bam.reference_range(bam.read_bai(p + '.bai')[0][1])
    inside = [k for k in range(len(offs)) if (vbeg >> 16) < offs[k] < (vend >> 16)]
    k = inside[len(inside) // 2]
    raw = bytearray(open(p, 'rb').read())
    blk = bytes(raw[offs[k]:offs[k] + sizes[k]])
    isize = int.from_bytes(blk[-4:], 'little')
    hit = None
    for byte in range(18, 18 + 40):                              # a header byte whose flip the host build refuses
        q = bytearray(blk)
        q[byte] ^= 0x10
        if ic.host_inflate(bytes(q[18:-8]), isize)[1] != 0:
            hit = byte
            break
    assert hit is not None
    raw[offs[k] + hit] ^= 0x10
    with open(p, 'wb') as f:
        f.write(bytes(raw))
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / 'o'), verbose=False, inflate='device')
    with pytest.raises(ValueError) as e:
        proc.load_chromosome_reads(chrom)
    assert p in str(e.value) and 'byte {0}'.format(int(offs[k])) in str(e.value) and 'does not inflate' in str(e.value)
    host = bam.NativeBamReadsProcessor(p, p + '.bai', output_dir=str(tmp_path / 'h'), verbose=False)
    pd.testing.assert_frame_equal(proc.load_chromosome_reads('chrG'), host.load_chromosome_reads('chrG'))
    assert len(proc.load_chromosome_reads('chrG')) == len(good)


def test_append_resident_needs_a_window():
    from degnorm_amd import _lib
    rows = bam.DeviceRows(0, True, False)
    try:
        with pytest.raises(_lib.DegnormAmdError, match='no resident window'):
            rows.append_resident(np.array([0], np.int64))
    finally:
        rows.close()


def test_pipeline_with_device_inflate_equals_golden(tmp_path):
    import _gtf_fixtures as gf
    from test_annotation_host import RUN_COLS, assert_same_table, golden_frame
    from test_gpu_pipeline import GTF, ITER, NMF_ITER, RESULT_FILES, assert_same_cov, golden_inputs
    from degnorm_amd.nmf import GeneNMFOA
    from degnorm_amd.pipeline import run_pipeline
    paths = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        p = str(tmp_path / (s + '.bam'))
        bf.write_bam(p, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1), level=6 if k == 2 else 1)
        paths.append(p)
    z = golden('pipeline')
    minimax, dropped = int(z['case_a_minimax']), z['case_a_dropped'].tolist()
    cov_e, genes_e, counts_e, samples = golden_inputs(z, dropped)
    out = str(tmp_path / 'out')
    os.makedirs(out)
    model, estimates, cov, counts_df, genes_df, exon_df, sample_ids = run_pipeline(
        paths, [p + '.bai' for p in paths], GTF, out, degnorm_iter=ITER, nmf_iter=NMF_ITER, minimax_coverage=minimax, verbose=False,
        inflate='device')
    assert sample_ids == samples
    assert_same_table(exon_df, golden_frame(z, 'exon', RUN_COLS))
    assert_same_table(genes_df, genes_e)
    assert_same_table(counts_df, counts_e)
    assert_same_cov(cov, cov_e)
    ref = GeneNMFOA(degnorm_iter=ITER, nmf_iter=NMF_ITER)
    est_e = ref.run(cov_e, reads_dat=counts_e[samples].values.astype(np.float64))
    np.testing.assert_array_equal(model.rho, ref.rho)
    np.testing.assert_array_equal(model.x_adj, ref.x_adj)
    for a, b in zip(estimates, est_e):
        np.testing.assert_array_equal(a, b)
    assert all(os.path.isfile(os.path.join(out, name)) for name in RESULT_FILES)

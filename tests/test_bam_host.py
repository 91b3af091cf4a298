"""
Host side of the native BAM reader (degnorm_amd.bam), no device: BGZF walk and EOF detection, framing through the
library's host export, header and .bai parsing (the three samtools indexes of the reference's test data), the pair order
against pandas and the paired check.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
from degnorm_amd import bam                                    # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REFS = [('c1', 200000), ('c2', 100000), ('c3', 5000)]


def _reads(n, seed=0, refs=(0, 1)):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({'ref': rng.choice(list(refs), n), 'pos': rng.integers(0, 90000, n),
                         'qname': ['r{0}'.format(i) for i in range(n)],
                         'cigar': rng.choice(['50M', '20M100N30M', '5S40M5S', '10M2I10M1D18M'], n)})


def _inflate_all(path):
    return b''.join(bam.inflate_block(b) for _, b in bam.iter_blocks(path))


@pytest.mark.parametrize('straddle', [False, True])
def test_bgzf_walk_and_eof(tmp_path, straddle):
    p = str(tmp_path / 's.bam')
    bf.write_bam(p, REFS, _reads(5000), straddle=straddle)
    off, size, isize = bam.bgzf_blocks(p)
    assert off[0] == 0 and np.all(off[1:] == off[:-1] + size[:-1]) and off[-1] + size[-1] == os.path.getsize(p)
    assert isize[-1] == 0 and size[-1] == 28 and isize.max() <= 65536
    assert bam.has_eof_block(p)
    data = _inflate_all(p)
    assert len(data) == isize.sum()
    cut = str(tmp_path / 'cut.bam')
    with open(p, 'rb') as f, open(cut, 'wb') as g:
        g.write(f.read()[:int(off[len(off) // 2]) + 100])           # in the middle of a block
    assert not bam.has_eof_block(cut)
    with pytest.raises(ValueError, match='truncated'):
        bam.bgzf_blocks(cut)


def test_truncated_file_refused_by_processor(tmp_path):
    p = str(tmp_path / 's.bam')
    bf.write_bam(p, REFS, _reads(2000))
    with open(p, 'rb') as f:
        raw = f.read()
    with open(p, 'wb') as f:
        f.write(raw[:-28])                                          # cut at a block boundary: only the EOF block is gone
    with pytest.raises(ValueError, match='end-of-file'):
        bam.NativeBamReadsProcessor(p, p + '.bai', verbose=False)


def test_header_parsing(tmp_path):
    p = str(tmp_path / 's.bam')
    bf.write_bam(p, REFS, _reads(100))
    assert bam.read_header(p) == REFS
    data = _inflate_all(p)
    end, refs = bam.parse_header(data)
    assert refs == REFS and end == len(bf.header_bytes(REFS))
    assert bam.parse_header(data[:end - 1]) is None
    with pytest.raises(ValueError, match='not a BAM'):
        bam.parse_header(b'BAI\x01' + data[4:])


@pytest.mark.parametrize('straddle', [False, True])
def test_framing_matches_writer_offsets_and_carries_the_tail(tmp_path, straddle):
    p = str(tmp_path / 's.bam')
    reads, offs, _ = bf.write_bam(p, REFS, _reads(3000, seed=2), straddle=straddle)
    data = _inflate_all(p)
    h = bam.parse_header(data)[0]
    rec = data[h:]
    off, used, _ = bam.frame_records(rec)
    np.testing.assert_array_equal(off, offs)
    assert used == len(rec)
    # a window end inside a record: the framed records stop before it, the rest is carried into the next window
    for cut in (int(offs[1000]) + 7, int(offs[1000]) + 2, int(offs[2000])):
        a, used_a, _ = bam.frame_records(rec[:cut])
        assert used_a == int(offs[np.searchsorted(offs, cut, side='right') - 1]) if cut not in offs.tolist() else used_a == cut
        b, used_b, _ = bam.frame_records(rec[used_a:])
        np.testing.assert_array_equal(np.concatenate([a, b + used_a]), offs)
        assert used_a + used_b == len(rec)


def test_framing_checks_order_and_reference(tmp_path):
    p = str(tmp_path / 's.bam')
    reads, offs, _ = bf.write_bam(p, REFS, _reads(500, refs=(0,)))
    data = _inflate_all(p)
    rec = data[bam.parse_header(data)[0]:]
    off, used, last = bam.frame_records(rec, 0)
    assert len(off) == 500 and last == int(reads.pos.iloc[-1])
    with pytest.raises(ValueError, match='refID'):
        bam.frame_records(rec, 1)
    with pytest.raises(ValueError, match='not sorted'):
        bam.frame_records(rec, 0, last_pos=int(reads.pos.iloc[0]) + 1)
    swapped = rec[int(offs[1]):int(offs[2])] + rec[:int(offs[1])]   # a later record first
    if reads.pos.iloc[1] > reads.pos.iloc[0]:
        with pytest.raises(ValueError, match='not sorted'):
            bam.frame_records(swapped, 0)
    with pytest.raises(ValueError, match='malformed'):
        bam.frame_records(b'\x05\x00\x00\x00' + b'\x00' * 40)


@pytest.mark.parametrize('name,beg,end,mapped', [('ff_small', 318, 5697397, 241002), ('hg_small_1', 265, 6571019, 99973),
                                                 ('hg_small_2', 288, 5825161, 99973)])
def test_bai_of_samtools(name, beg, end, mapped):
    refs, n_no_coor = bam.read_bai(os.path.join(GOLDEN, name + '.bai'))
    assert len(refs) == 1 and n_no_coor == 0
    assert refs[0]['pseudo'] == (beg << 16, end << 16, mapped, 0)
    assert bam.reference_range(refs[0]) == (beg << 16, end << 16)
    assert refs[0]['chunk_min'] == beg << 16 and refs[0]['chunk_max'] <= end << 16


def test_bai_of_writer_and_fallbacks(tmp_path):
    p = str(tmp_path / 's.bam')
    reads, offs, _ = bf.write_bam(p, REFS, _reads(3000, refs=(0, 1)))
    refs, n_no_coor = bam.read_bai(p + '.bai')
    assert len(refs) == 3 and n_no_coor == 0
    assert refs[0]['pseudo'][2] == (reads.ref == 0).sum() and refs[2]['pseudo'] is None and refs[2]['n_bin'] == 0
    assert bam.reference_range(refs[2]) is None
    no_pseudo = dict(refs[1], pseudo=None)
    assert bam.reference_range(no_pseudo) == (refs[1]['chunk_min'], refs[1]['chunk_max']) == refs[1]['pseudo'][:2]


def test_pair_order_equals_pandas_sort_values():
    rng = np.random.default_rng(5)
    n = 120000
    stems = np.array(['p', 'pa', 'pab', 'pair.x', 'SRR1.', 'q'])
    keys = [str(stems[rng.integers(0, len(stems))]) + str(int(rng.integers(0, 40000))) for _ in range(n)]
    keys[::97] = [''] * len(keys[::97])                           # names without a dot
    df = pd.DataFrame({'qname_unpaired': keys, 'row': np.arange(n)})
    expect = df.sort_values('qname_unpaired')['row'].values
    width = max(len(k) for k in keys)
    order, pair_id, n_ids = bam.pair_order(np.array([k.encode() for k in keys], dtype='S{0}'.format(width)))
    np.testing.assert_array_equal(order, expect)
    sk = np.array(keys, dtype=object)[order]
    assert n_ids == len(set(keys))
    assert np.all((pair_id[1:] != pair_id[:-1]) == (sk[1:] != sk[:-1])) and pair_id[0] == 0


def test_paired_check_reads_the_first_301_records(tmp_path):
    n = 600
    qn = ['f{0}.{1}'.format(i // 2, 1 + i % 2) for i in range(n)]
    for k in (301, 400):                                            # beyond the first 301: not looked at
        qn[k] = 'odd{0}'.format(k)
    reads = pd.DataFrame({'ref': 0, 'pos': np.arange(n) * 10, 'qname': qn, 'cigar': '50M', 'next_ref': 0})
    p = str(tmp_path / 'pe.bam')
    bf.write_bam(p, REFS, reads)
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', verbose=False)
    assert proc.paired and proc.chroms == ['c1', 'c2', 'c3']
    assert proc.header.chr.tolist() == ['c1', 'c2', 'c3'] and proc.header.length.tolist() == [200000, 100000, 5000]
    assert proc.sample_id == 'pe' and proc.save_dir == os.path.join(str(tmp_path), 'tmp', 'pe')
    assert len(proc._leading_query_names('c1')) == 301
    qn[300] = 'odd300'
    reads['qname'] = qn
    bf.write_bam(p, REFS, reads)
    assert not bam.NativeBamReadsProcessor(p, p + '.bai', chroms=['c1', 'cX'], verbose=False).paired


def test_constructor_checks(tmp_path):
    p = str(tmp_path / 's.bam')
    bf.write_bam(p, REFS, _reads(50))
    with pytest.raises(ValueError, match='.bai'):
        os.rename(p + '.bai', p + '.idx')
        bam.NativeBamReadsProcessor(p, p + '.idx', verbose=False)
    with pytest.raises(FileNotFoundError):
        bam.NativeBamReadsProcessor(p, p + '.bai', verbose=False)
    with pytest.raises(ValueError, match='not a .bam'):
        bam.NativeBamReadsProcessor(p + '.idx', p + '.idx', verbose=False)
    os.rename(p + '.idx', p + '.bai')
    proc = bam.NativeBamReadsProcessor(p, p + '.bai', chroms=['c2', 'c9'], verbose=False)
    assert proc.chroms == ['c2'] and not proc.paired and isinstance(proc, bam.BamReadsProcessor)

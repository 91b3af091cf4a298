"""
dn_assemble_coverage (csrc/dn_assemble.hip) through ctypes on random layouts, against `dense[idx] = val` in numpy, sliced and
concatenated; the comparison is exact (the values are whole numbers up to 2^24, float32 holds them).  No files: the samples'
CSR rows, the genes' intervals and the chunk table are made here.

Layouts: chromosomes of 1, 5000 and 70001 bases; 1, 3 and 5 samples, of which (from 3 on) one has every position set and the
next has none -- a dense vector that is not cleared between samples shows there; indices unsorted; genes of 1 and of 6
intervals whose lengths sit on both sides of the 256 threads of a block and of the chunk sizes 1, 1000 and 4096; intervals that
touch base 0 and the chromosome's end; the chunk table in random order.  Only sound tables reach the device: the refusals
of bad ones are tests/test_error_channel_host.py's.
"""
import ctypes

import numpy as np
import pytest

from degnorm_amd import _lib

pytestmark = pytest.mark.gpu

INTERVAL_LENGTHS = (1, 255, 256, 257, 4095, 4096, 4097)


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def samples(rng, chrom_len, p):
    """[(indices int32 unsorted, values float32)] per sample: sparse, every position, none, sparse, every position."""
    out = []
    for i in range(p):
        kind = ('sparse', 'full', 'none')[i % 3] if p > 1 else ('full' if chrom_len % 2 else 'sparse')
        k = {'full': chrom_len, 'none': 0}.get(kind, int(rng.integers(1, max(2, chrom_len // 3 + 1))))
        idx = rng.permutation(chrom_len)[:k].astype(np.int32)
        out.append((idx, rng.integers(1, 2 ** 24 + 1, k).astype(np.float32)))
    return out


def genes(rng, chrom_len):
    """Per gene a list of (start, end): 1 or 6 intervals in ascending order; the first gene starts at base 0, the second ends
    with the chromosome, every interval length of the list occurs (cut to the chromosome)."""
    lengths = [min(L, chrom_len) for L in INTERVAL_LENGTHS]
    out = []
    for g in range(8):
        k = 6 if g % 2 else 1
        ivs = []
        for j in range(k):
            L = lengths[(g + j) % len(lengths)]
            a = int(rng.integers(0, chrom_len - L + 1))
            ivs.append((a, a + L))
        ivs.sort()
        if g == 0:
            ivs[0] = (0, ivs[0][1] - ivs[0][0])
        if g in (1, 2):
            a, b = ivs[-1]
            ivs[-1] = (chrom_len - (b - a), chrom_len)
        out.append(ivs)
    return out


def chunk_table(rng, gene_ivs, chunk):
    rows = []
    for g, ivs in enumerate(gene_ivs):
        col = 0
        for a, b in ivs:
            for s0 in range(a, b, chunk):
                ln = min(chunk, b - s0)
                rows.append((g, s0, col, ln))
                col += ln
    rows = [rows[k] for k in rng.permutation(len(rows))]
    g, s, d, l = zip(*rows)
    return np.array(g, np.int32), np.array(s, np.int64), np.array(d, np.int64), np.array(l, np.int32)


def reference(chrom_len, smp, gene_ivs):
    dense = np.zeros((len(smp), chrom_len), np.float32)
    for i, (idx, val) in enumerate(smp):
        dense[i, idx] = val
    return np.concatenate([np.concatenate([dense[:, a:b] for a, b in ivs], axis=1).reshape(-1) for ivs in gene_ivs])


@pytest.mark.parametrize('chunk', (1, 1000, 4096))
@pytest.mark.parametrize('p', (1, 3, 5))
@pytest.mark.parametrize('chrom_len', (1, 5000, 70001))
def test_random_layout(chrom_len, p, chunk):
    rng = np.random.default_rng(chrom_len * 100 + p * 10 + chunk % 7)
    smp, gene_ivs = samples(rng, chrom_len, p), genes(rng, chrom_len)
    lengths = np.array([sum(b - a for a, b in ivs) for ivs in gene_ivs], np.int64)
    c_gene, c_src, c_dst, c_len = chunk_table(rng, gene_ivs, chunk)
    assert min(a for ivs in gene_ivs for a, _ in ivs) == 0 and max(b for ivs in gene_ivs for _, b in ivs) == chrom_len
    assert {len(ivs) for ivs in gene_ivs} == {1, 6}
    assert {b - a for ivs in gene_ivs for a, b in ivs} == {min(L, chrom_len) for L in INTERVAL_LENGTHS}
    if p >= 3:
        assert smp[1][0].size == chrom_len and smp[2][0].size == 0
    assert all(np.any(np.diff(idx) < 0) for idx, _ in smp if idx.size > 10)              # unsorted

    nnz = np.array([idx.size for idx, _ in smp], np.int64)
    iptrs = (ctypes.c_void_p * p)(*[idx.ctypes.data if idx.size else None for idx, _ in smp])
    vptrs = (ctypes.c_void_p * p)(*[val.ctypes.data if val.size else None for _, val in smp])
    out = np.full(int(lengths.sum()) * p, -1.0, np.float32)
    lib = _lib.load()
    rc = lib.dn_assemble_coverage(0, chrom_len, p, _ptr(nnz), iptrs, vptrs, len(gene_ivs), _ptr(lengths), c_gene.size, _ptr(c_gene),
                                  _ptr(c_src), _ptr(c_dst), _ptr(c_len), _ptr(out), None)
    assert rc == _lib.DN_OK, lib.dn_assemble_last_error()
    want = reference(chrom_len, smp, gene_ivs)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, '{0} of {1} values differ, first at {2}: device {3}, numpy {4}'.format(bad.size, out.size, bad[0], out[bad[0]], want[bad[0]])

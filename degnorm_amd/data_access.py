"""
Raw and DegNorm-estimated coverage curves out of an output directory (reference: `degnorm/data_access.py`).

    python -m degnorm_amd.data_access -d DEGNORM_DIR -g GENE [GENE ...] | all -o SAVE_DIR [--device K] [--formatter pandas]

get_coverage_data(genes, degnorm_dir, save_dir) returns the reference's nested dict of L x p DataFrames and, with save_dir,
writes <save_dir>/<chr>/<GENE>_raw_coverage.txt and <GENE>_estimated_coverage.txt, which the reference writes through
`DataFrame(cov.T, columns=sample_ids).to_csv(file, index=None, sep=' ', float_format='%.5f')`.  The cost of that call is its
number formatting, about half a million values a second.  Here the bodies of the files are formatted on the GPU
(csrc/dn_text.hip; include/degnorm_amd.h, "Coverage matrices to text", states the rule that reproduces '%.5f' exactly): the
matrices of a batch of genes go up once, the text of all their files comes back as one pinned buffer, and the files are
written from slices of it behind a header line that pandas itself formats.  The files equal the reference's byte for byte.
A gene that holds a NaN, an infinity or a value of 2^63 and more is flagged by the device and written through pandas.
formatter='pandas' is the reference's writer for every gene.  There is no CPU fallback for the call as a whole: the device
formatter without a device raises.

The directories that run_pipeline and run_from_warm_start write are valid inputs.  Not offered: get_coverage_plots.
"""
import argparse
import ctypes
import io
import os
import pickle
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from pandas import DataFrame, read_csv

from . import _lib

REQUIRED_FILES = ('gene_exon_metadata.csv', 'read_counts.csv', 'degradation_index_scores.csv')
BATCH_BYTES = 256 << 20                 # float64 bytes of the matrices of one device batch (its text is about as large)


class CoverageLoader(object):
    """Coverage matrices and exon positions of a set of genes of a DegNorm output directory."""

    def __init__(self, data_dir):
        self.genes = None
        self.chroms = None
        self.sample_ids = None
        self.exon_df = None
        self.cov_dict = dict()
        if not os.path.isdir(data_dir):
            raise NotADirectoryError('{0} is not a directory, cannot find DegNorm output.'.format(data_dir))
        self.data_dir = data_dir
        if not all(os.path.isfile(os.path.join(data_dir, f)) for f in REQUIRED_FILES):
            raise ValueError('Missing requested files. Check that {0} is a  DegNorm output directory.'.format(data_dir))

    def load(self, genes):
        """genes: a gene name, a list of names, or 'all' (any letter case); names are case-insensitive."""
        all_genes = isinstance(genes, str) and genes.lower() == 'all'
        if isinstance(genes, str):
            genes = [genes]
        self.exon_df = read_csv(os.path.join(self.data_dir, 'gene_exon_metadata.csv'), low_memory=False)
        with open(os.path.join(self.data_dir, 'degradation_index_scores.csv'), 'r') as di:
            self.sample_ids = di.readline().strip().split(',')[2:]
        if all_genes:
            genes = self.exon_df.gene.unique().tolist()
        self.genes = [str(g).upper() for g in genes]
        self.exon_df.gene = self.exon_df.gene.apply(lambda g: g.upper())
        if not all_genes:
            missing = sorted(set(self.genes) - set(self.exon_df.gene.unique()))
            if missing:
                raise ValueError('Genes {0} were not found in DegNorm output. Check that they were run through pipeline.'
                                 .format(', '.join(missing)))
            self.exon_df = self.exon_df[self.exon_df.gene.isin(self.genes)]
        self.chroms = self.exon_df.chr.unique().tolist()
        for chrom in self.chroms:
            mats = []
            for name in ('coverage_matrices_{0}.pkl', 'estimated_coverage_matrices_{0}.pkl'):
                with open(os.path.join(self.data_dir, str(chrom), name.format(chrom)), 'rb') as f:
                    mats.append({k.upper(): v for k, v in pickle.load(f).items()})
            for gene in self.exon_df[self.exon_df.chr == chrom].gene.unique():
                raw, est = mats[0].get(gene), mats[1].get(gene)
                if raw is not None and est is not None:
                    self.cov_dict[gene] = {'raw': raw, 'estimate': est}
        return self


# -- the device formatter ------------------------------------------------------------------------------------------------

class CovText(object):
    """The text of one batch of matrices: `off` (n + 1 offsets), `flag` (n, 1: not formatted, empty piece) and the bytes, which
    live in the library until close()."""

    def __init__(self, lib, handle, off, flag, ms):
        self.lib, self.h, self.off, self.flag, self.ms = lib, handle, off, flag, ms
        n = int(lib.dn_text_size(handle))
        self.size = n
        self.view = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(lib.dn_text_bytes(handle))) if n else np.zeros(0, np.uint8)

    def piece(self, k):
        """A view of the library's memory: not to be used after close()."""
        return self.view[int(self.off[k]):int(self.off[k + 1])]

    def close(self):
        if self.h is not None:
            self.view = None
            self.lib.dn_text_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _batch_arrays(mats):
    mats = [np.asarray(m) for m in mats]
    if not mats:
        raise ValueError('no matrices')
    if any(m.ndim != 2 for m in mats):
        raise ValueError('Not all coverage matrices are 2-d arrays!')
    p = int(mats[0].shape[0])
    if any(m.shape[0] != p for m in mats):
        raise ValueError('coverage matrices disagree on the number of samples')
    lens = np.array([m.shape[1] for m in mats], dtype=np.int64)
    beg = np.concatenate([[0], np.cumsum(lens * p)]).astype(np.int64)
    x = np.empty(max(int(beg[-1]), 1), dtype=np.float64)
    for m, b in zip(mats, beg):
        x[b:b + m.size] = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    return x, beg[:-1].copy(), lens, p


def cov_text(mats, device=None, host=False):
    """One batch through dn_cov_text (host=True: dn_cov_text_host, the host build of the same source): a CovText.
    mats: p x L_g matrices, one p.  The caller closes the result."""
    lib = _lib.load()
    x, beg, lens, p = _batch_arrays(mats)
    n = len(lens)
    off = np.zeros(n + 1, dtype=np.int64)
    flag = np.zeros(n, dtype=np.uint8)
    ms = np.zeros(5)
    h = ctypes.c_void_p()
    args = [_lib._p(x, ctypes.c_double), x.size, n, p, _lib._p(beg, ctypes.c_int64), _lib._p(lens, ctypes.c_int64),
            _lib._p(off, ctypes.c_int64), _lib._p(flag, ctypes.c_uint8), ctypes.byref(h)]
    if host:
        _lib._check(lib.dn_cov_text_host(*args), 'dn_cov_text_host')
    else:
        dev = int(os.environ.get('LOCAL_RANK', 0)) if device is None else int(device)
        _lib._check(lib.dn_cov_text(dev, *(args + [_lib._p(ms, ctypes.c_double)])), 'dn_cov_text')
    return CovText(lib, h, off, flag, ms)


def batch_cuts(sizes, batch_bytes):
    """[lo, hi) index ranges: a batch is closed by the matrix that brings its float64 bytes to batch_bytes."""
    cuts, lo, held = [], 0, 0
    for k, s in enumerate(sizes):
        held += 8 * int(s)
        if held >= batch_bytes:
            cuts.append((lo, k + 1))
            lo, held = k + 1, 0
    if lo < len(sizes):
        cuts.append((lo, len(sizes)))
    return cuts


def cov_text_pieces(mats, device=None, host=False, batch_bytes=BATCH_BYTES):
    """(the bytes of every matrix's piece, the flags, the number of batches) with the matrices cut into batches."""
    mats = list(mats)
    pieces, flags = [], []
    cuts = batch_cuts([np.asarray(m).size for m in mats], batch_bytes)
    for lo, hi in cuts:
        with cov_text(mats[lo:hi], device=device, host=host) as t:
            pieces += [bytes(t.piece(k)) for k in range(hi - lo)]
            flags += t.flag.tolist()
    return pieces, np.array(flags, dtype=np.uint8), len(cuts)


# -- get_coverage_data ---------------------------------------------------------------------------------------------------

def header_line(sample_ids):
    """The first line of a file, as pandas writes it (an id that holds the separator is quoted)."""
    s = io.StringIO()
    DataFrame(columns=list(sample_ids)).to_csv(s, index=None, sep=' ', float_format='%.5f')
    return s.getvalue().encode('utf-8')


def _write_pandas(path, df):
    df.to_csv(path, index=None, sep=' ', float_format='%.5f')


def _write_piece(path, header, piece):
    with open(path, 'wb') as f:
        f.write(header)
        f.write(piece)


def get_coverage_data(genes, degnorm_dir, save_dir=None, device=None, n_jobs=1, formatter='device', batch_bytes=BATCH_BYTES,
                      stats=None):
    """
    Raw and DegNorm-estimated coverage of a set of genes of a DegNorm output directory.

    :param genes: str or list of str, gene names (case insensitive), or 'all'
    :param degnorm_dir: output directory of a DegNorm run
    :param save_dir: if given, every gene's matrices are written to save_dir/<chr>/<GENE>_raw_coverage.txt and
     save_dir/<chr>/<GENE>_estimated_coverage.txt (base positions x samples, '%.5f', separated by spaces)
    :param device: GPU of the 'device' formatter (None: LOCAL_RANK or 0)
    :param n_jobs: threads that write files from the text of a batch
    :param formatter: 'device' (the text is formatted on the GPU) or 'pandas' (the reference's to_csv call)
    :param batch_bytes: float64 bytes of the matrices that go to the device at a time
    :param stats: a dict that receives seconds (load, format_call, write, pandas) and device milliseconds (upload_ms, measure_ms,
     scan_ms, emit_ms, copy_back_ms), values, text_bytes, batches and flagged_files
    :return: dict gene -> {'raw': DataFrame, 'estimate': DataFrame}, L x p with the sample ids as columns
    """
    if formatter not in ('device', 'pandas'):
        raise ValueError('formatter must be "device" or "pandas"')
    st = {k: 0.0 for k in ('load', 'format_call', 'write', 'pandas', 'upload_ms', 'measure_ms', 'scan_ms', 'emit_ms', 'copy_back_ms')}
    st.update(values=0, text_bytes=0, batches=0, flagged_files=0)
    t0 = time.perf_counter()
    ldr = CoverageLoader(degnorm_dir).load(genes)
    st['load'] = time.perf_counter() - t0
    out = dict()
    for gene, cov in ldr.cov_dict.items():
        out[gene] = {'raw': DataFrame(cov['raw'].T, columns=ldr.sample_ids), 'estimate': DataFrame(cov['estimate'].T, columns=ldr.sample_ids)}
    if save_dir:
        chrom_of = ldr.exon_df.drop_duplicates('gene').set_index('gene').chr.astype(str)
        files = []                                             # (path, matrix, frame), two a gene, in the reference's order
        for gene, cov in ldr.cov_dict.items():
            cdir = os.path.join(save_dir, chrom_of[gene])
            os.makedirs(cdir, exist_ok=True)
            files.append((os.path.join(cdir, '{0}_raw_coverage.txt'.format(gene)), cov['raw'], out[gene]['raw']))
            files.append((os.path.join(cdir, '{0}_estimated_coverage.txt'.format(gene)), cov['estimate'], out[gene]['estimate']))
        st['values'] = int(sum(np.asarray(m).size for _, m, _ in files))
        if formatter == 'pandas':
            t0 = time.perf_counter()
            for path, _, df in files:
                _write_pandas(path, df)
            st['pandas'] = time.perf_counter() - t0
        elif files:
            header = header_line(ldr.sample_ids)
            with ThreadPoolExecutor(max_workers=max(1, int(n_jobs))) as pool:
                for lo, hi in batch_cuts([np.asarray(m).size for _, m, _ in files], batch_bytes):
                    t0 = time.perf_counter()
                    with cov_text([m for _, m, _ in files[lo:hi]], device=device) as t:
                        t1 = time.perf_counter()
                        jobs = [pool.submit(_write_piece, files[lo + k][0], header, t.piece(k)) for k in range(hi - lo) if not t.flag[k]]
                        for j in jobs:
                            j.result()
                        t2 = time.perf_counter()
                        for k in np.flatnonzero(t.flag):            # NaN, infinities, 2^63 and more: the reference's writer
                            _write_pandas(files[lo + k][0], files[lo + k][2])
                        st['pandas'] += time.perf_counter() - t2
                        st['format_call'] += t1 - t0
                        st['write'] += t2 - t1
                        for key, v in zip(('upload_ms', 'measure_ms', 'scan_ms', 'emit_ms', 'copy_back_ms'), t.ms):
                            st[key] += float(v)
                        st['text_bytes'] += t.size
                        st['batches'] += 1
                        st['flagged_files'] += int(t.flag.sum())
    if stats is not None:
        stats.update(st)
    return out


def argparser():
    ap = argparse.ArgumentParser(prog='python -m degnorm_amd.data_access',
                                 description='Write raw and DegNorm-estimated coverage of genes of a DegNorm output directory as text files.',
                                 epilog='Not offered: coverage plots (get_coverage_plots, --plot-genes) and the HTML report.')
    ap.add_argument('-d', '--degnorm-dir', required=True, help='output directory of a DegNorm run')
    ap.add_argument('-g', '--genes', nargs='+', required=True, help='gene names (case insensitive), or the word all')
    ap.add_argument('-o', '--save-dir', required=True, help='directory the files are written under, <chr>/<GENE>_raw_coverage.txt and '
                                                             '<chr>/<GENE>_estimated_coverage.txt')
    ap.add_argument('--device', type=int, default=None, help='GPU that formats the text (default: LOCAL_RANK or 0)')
    ap.add_argument('--formatter', choices=('device', 'pandas'), default='device', help='pandas: the reference\'s to_csv call, no GPU')
    ap.add_argument('-c', '--cpus', type=int, default=1, help='threads that write files')
    return ap


def main(argv=None):
    args = argparser().parse_args(argv)
    genes = 'all' if len(args.genes) == 1 and args.genes[0].lower() == 'all' else args.genes
    stats = {}
    out = get_coverage_data(genes, args.degnorm_dir, save_dir=args.save_dir, device=args.device, n_jobs=args.cpus, formatter=args.formatter,
                            stats=stats)
    print('{0} genes, {1} values written under {2}'.format(len(out), stats['values'], args.save_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())

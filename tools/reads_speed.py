"""
Speed of the reads -> coverage / read counts path (dn_read_coverage) on the synthetic scale chromosome of the GPU tests
(tests/_reads_fixtures.scale_case: 20 Mb, 2 000 genes, 2 M single-end reads of the forms aM / aMnNbM):

  device_ms      device time of the call (prefilter, per-read kernel, scans, CSR select; events on its stream)
  pack_ms        host packing of the reads (CIGAR bytes + offsets) and the annotation
  call_ms        the whole dn_read_coverage call (uploads, kernels, downloads)
  reads_per_s    end to end: reads / (pack + call + result assembly), the rate chromosome_coverage_read_counts_df gives

    python tools/reads_speed.py [--reads 2000000] [--chrom-len 20000000] [--reps 3]

Prints one JSON line.  Needs a GPU.  The reference (degnorm/reads.py:314-818, one Python loop over the reads) is not on the
GPU machine; its rate, measured on one CPU core with the same generator shrunk to 200 000 reads over 2 Mb (200 genes), is
REFERENCE_READS_PER_S below (python 3, numpy, pandas; the isolated-stage loop dominates).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _reads_fixtures as rf                         # noqa: E402
from degnorm_amd import reads as dr                  # noqa: E402

REFERENCE_READS_PER_S = 37400                 # 200 000 reads in 5.35 s on one core: 37 376 reads/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=2_000_000)
    ap.add_argument('--chrom-len', type=int, default=20_000_000)
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case(chrom_len=a.chrom_len, n_genes=a.genes, n_reads=a.reads)
    best = None
    for _ in range(a.reps + 1):                      # the first call loads the library and warms the device up
        t0 = time.perf_counter()
        ann = dr.Annotation(chrom_len, ov, gene_df, exon_df)
        packed = dr.pack_reads(reads, False)
        t1 = time.perf_counter()
        counts, ol_cov, idx, val, n_iso, dev_ms = dr.device_read_coverage(*packed, ann, False)
        t2 = time.perf_counter()
        t_e2e = time.perf_counter()
        dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, False)
        e2e = time.perf_counter() - t_e2e
        row = {'device_ms': dev_ms, 'pack_ms': 1e3 * (t1 - t0), 'call_ms': 1e3 * (t2 - t1), 'e2e_ms': 1e3 * e2e}
        if best is None or row['e2e_ms'] < best['e2e_ms']:
            best = row
    out = {'tool': 'reads_speed', 'reads': a.reads, 'chrom_len': chrom_len, 'genes': len(gene_df),
           'nnz': int(idx.size), 'counted': int(counts.sum()),
           'device_ms': round(best['device_ms'], 3), 'pack_ms': round(best['pack_ms'], 1), 'call_ms': round(best['call_ms'], 1),
           'e2e_ms': round(best['e2e_ms'], 1), 'device_reads_per_s': round(a.reads / (best['device_ms'] * 1e-3)),
           'reads_per_s': round(a.reads / (best['e2e_ms'] * 1e-3)), 'reference_reads_per_s_cpu': REFERENCE_READS_PER_S}
    print(json.dumps(out))


if __name__ == '__main__':
    main()

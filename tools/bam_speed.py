"""
Speed of the native BAM path (degnorm_amd.bam.NativeBamReadsProcessor) on the synthetic scale chromosome of the GPU tests
(tests/_reads_fixtures.scale_case: 20 Mb, 2 000 genes, 2 M single-end reads of the forms aM / aMnNbM), written as a sorted,
indexed BAM, and on a paired variant (the same reads named <i // 2>.1 / .2, mates next to each other):

  inflate_ms        host BGZF inflate of the chromosome's blocks (n_jobs threads)
  frame_ms          host record framing (dn_bam_frame)
  decode_ms         the append calls: window upload, decode / filter kernels, compaction into the row store
  coverage_ms       the coverage call on the stored rows (paired: with the key download and the host sort)
  coverage_device_ms  device time of the coverage stages (events on its stream)
  reads_per_s       end to end: reads / chromosome_coverage_read_counts (files written, index and header already read)
  in_memory_reads_per_s  chromosome_coverage_read_counts_df on the same reads held as a DataFrame

    python tools/bam_speed.py [--reads 2000000] [--jobs 4] [--reps 3] [--dir DIR]

Prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                                   # noqa: E402
import pandas as pd                                  # noqa: E402

import _bam_fixtures as bf                           # noqa: E402
import _reads_fixtures as rf                         # noqa: E402
from degnorm_amd import bam                          # noqa: E402
from degnorm_amd import reads as dr                  # noqa: E402


def _best(path, chrom, ov, gene_df, exon_df, out, jobs, reps):
    best = None
    for k in range(reps + 1):                        # the first run loads the library and warms the device up
        proc = bam.NativeBamReadsProcessor(path, path + '.bai', output_dir=os.path.join(out, str(k)), n_jobs=jobs, verbose=False)
        os.makedirs(proc.save_dir, exist_ok=True)
        proc.timing = {}
        t0 = time.perf_counter()
        proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
        e2e = time.perf_counter() - t0
        t = proc.timing
        row = {'inflate_ms': 1e3 * t.get('inflate_s', 0), 'frame_ms': 1e3 * t.get('frame_s', 0), 'decode_ms': 1e3 * t.get('decode_s', 0),
               'coverage_ms': 1e3 * t.get('coverage_s', 0), 'coverage_device_ms': t.get('coverage_device_ms', 0), 'e2e_ms': 1e3 * e2e}
        if k > 0 and (best is None or row['e2e_ms'] < best['e2e_ms']):
            best = row
    return {key: round(v, 1 if key != 'coverage_device_ms' else 3) for key, v in best.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=2_000_000)
    ap.add_argument('--jobs', type=int, default=4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--dir', default=None)
    a = ap.parse_args()
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case(n_reads=a.reads)
    work = a.dir or tempfile.mkdtemp(prefix='bam_speed_')
    try:
        se = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
        pe = se.assign(qname=['{0}.{1}'.format(i // 2, 1 + i % 2) for i in range(len(se))], next_ref=0)
        t0 = time.perf_counter()
        bf.write_bam(os.path.join(work, 'se.bam'), [('chrS', chrom_len)], se)
        bf.write_bam(os.path.join(work, 'pe.bam'), [('chrS', chrom_len)], pe)
        write_s = time.perf_counter() - t0
        in_mem = None
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, False)
            dt = time.perf_counter() - t0
            in_mem = dt if in_mem is None else min(in_mem, dt)
        out = {'tool': 'bam_speed', 'reads': a.reads, 'jobs': a.jobs, 'bam_mb': round(os.path.getsize(os.path.join(work, 'se.bam')) / 2 ** 20, 1),
               'write_s': round(write_s, 1)}
        for name in ('se', 'pe'):
            row = _best(os.path.join(work, name + '.bam'), 'chrS', ov, gene_df, exon_df, os.path.join(work, 'out_' + name),
                        a.jobs, a.reps)
            row['reads_per_s'] = round(a.reads / (row['e2e_ms'] * 1e-3))
            out[name] = row
        out['in_memory_ms'] = round(1e3 * in_mem, 1)
        out['in_memory_reads_per_s'] = round(a.reads / in_mem)
        print(json.dumps(out))
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

"""
Speed of the GFF3 scan (degnorm_amd.loaders.Gff3AnnotationLoader, csrc/dn_gff3.hip) against the GTF scan on the same
annotation: the seeded GTF of tests/_gtf_fixtures.write_gtf (default about 1.5 GB, 5 M lines) and its three GFF3 twins of
tests/_gff3_fixtures.write_gff3 (`gencode`, `ensembl`, `ncbi`).  After one warm-up load of each kind on small files the four
files are loaded in turn, --reps times round after round, and every load prints one JSON line:

  device_ms         the scanner's kernels, all windows (HIP events)
  resolve_ms        GFF3 only: the sort of the node rows and the walk of the exons that named a Parent (HIP events)
  scan_ms           device_ms + resolve_ms: what is held against the GTF twin's device_ms
  copy_in_ms, read_s, codes_s (exon_codes() end to end, interning of the names included), nodes, walked_exons

and a last line has the minimum and maximum of scan_ms per file and the ratio to the GTF file's.

    python tools/gff3_speed.py [--bytes 1572864000] [--reps 5] [--window-bytes 268435456] [--dir DIR]

Needs a GPU.
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

import _gff3_fixtures as g3                          # noqa: E402
import _gtf_fixtures as gf                           # noqa: E402
from degnorm_amd import loaders                      # noqa: E402


def load(kind, path, window_bytes):
    ld = loaders.annotation_loader(path, window_bytes=window_bytes)
    t0 = time.perf_counter()
    codes = ld.exon_codes()
    codes_s = time.perf_counter() - t0
    t = ld.timing
    return {'file': kind, 'bytes': t['bytes'], 'lines': t['lines'], 'exon_lines': int(codes[0].size), 'genes': len(codes[5]),
            'device_ms': round(t['device_ms'], 2), 'resolve_ms': round(t.get('resolve_ms', 0.0), 2),
            'scan_ms': round(t['device_ms'] + t.get('resolve_ms', 0.0), 2), 'copy_in_ms': round(t['copy_ms'], 1),
            'read_s': round(t['read_s'], 3), 'codes_s': round(codes_s, 2), 'nodes': t.get('nodes', 0), 'walked_exons': t.get('walked_exons', 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=1500 << 20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window-bytes', type=int, default=loaders.WINDOW_BYTES)
    ap.add_argument('--dir', default=None)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix='gff3_speed_')
    try:
        for d in g3.DIALECTS:                        # warm-up: library load, code objects of both scanners and of the sort
            gtf, gff3 = g3.write_twin(work, 1, 2 << 20, d)
            loaders.annotation_loader(gtf).exon_codes()
            loaders.annotation_loader(gff3).exon_codes()
        t0 = time.perf_counter()
        files = [('gtf', os.path.join(work, 'seeded.gtf'))]
        _, n_genes, _ = gf.write_gtf(files[0][1], 7, a.bytes)
        for d in g3.DIALECTS:
            files.append(('gff3-' + d, os.path.join(work, 'seeded_{0}.gff3'.format(d))))
            g3.write_gff3(files[-1][1], 7, n_genes, d)
        print(json.dumps({'tool': 'gff3_speed', 'genes': n_genes, 'write_s': round(time.perf_counter() - t0, 1), 'window_bytes': a.window_bytes,
                          'reps': a.reps}), flush=True)
        seen = {k: [] for k, _ in files}
        for rep in range(a.reps):
            for kind, path in files:                 # round after round: drift of the machine falls on all four alike
                r = load(kind, path, a.window_bytes)
                seen[kind].append(r['scan_ms'])
                print(json.dumps(dict(r, rep=rep)), flush=True)
        base = min(seen['gtf'])
        print(json.dumps({'summary': {k: {'scan_ms_min': min(v), 'scan_ms_max': max(v), 'min_over_gtf_min': round(min(v) / base, 2)}
                                      for k, v in seen.items()}}), flush=True)
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

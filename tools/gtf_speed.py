"""
Speed of the annotation stage (degnorm_amd.loaders.GeneAnnotationLoader, degnorm_amd.gene_processing.GeneAnnotationProcessor)
on the seeded GENCODE-style GTF of tests/_gtf_fixtures.write_gtf at a size near a real human annotation (default about 1.5 GB,
5 M lines).  After one warm-up run on a small file (library load, code objects) it reports, as one JSON line:

  read_s            reading the file in windows (host, page cache warm: the generator has just written it)
  copy_in_ms        copies of the windows to the device (HIP events)
  scan_device_ms    the scanner's kernels (HIP events around them, all windows); scan_gbps = bytes / that time, next to the
                    HBM peak of the data sheet (8 000 GB/s) and the measured float4 copy rate (6 290 GB/s)
  get_data_s        GeneAnnotationLoader.get_data() end to end
  run_s             GeneAnnotationProcessor.run() end to end (its own load included)

    python tools/gtf_speed.py [--bytes 1572864000] [--window-bytes 268435456] [--dir DIR]

Needs a GPU.  The reference's time for the same seeded file comes from tests/golden/make_golden_pipeline.py --time on a host
that has the reference.
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

import _gtf_fixtures as gf                           # noqa: E402
from degnorm_amd import loaders                      # noqa: E402
from degnorm_amd.gene_processing import GeneAnnotationProcessor   # noqa: E402

HBM_PEAK_GBPS = 8000.0
HBM_COPY_GBPS = 6290.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=1500 << 20)
    ap.add_argument('--window-bytes', type=int, default=loaders.WINDOW_BYTES)
    ap.add_argument('--dir', default=None)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix='gtf_speed_')
    try:
        warm = os.path.join(work, 'warm.gtf')
        gf.write_gtf(warm, 1, 4 << 20)
        loaders.GeneAnnotationLoader(warm).get_data()
        path = os.path.join(work, 'seeded.gtf')
        t0 = time.perf_counter()
        n_lines, n_genes, size = gf.write_gtf(path, 7, a.bytes)
        write_s = time.perf_counter() - t0
        loaders.WINDOW_BYTES = a.window_bytes
        ld = loaders.GeneAnnotationLoader(path)
        t0 = time.perf_counter()
        df = ld.get_data()
        get_data_s = time.perf_counter() - t0
        t = dict(ld.timing)
        t0 = time.perf_counter()
        run_df = GeneAnnotationProcessor(path, verbose=False).run()
        run_s = time.perf_counter() - t0
        print(json.dumps({'tool': 'gtf_speed', 'bytes': size, 'lines': n_lines, 'genes': n_genes, 'exon_rows': int(len(df)),
                          'run_rows': int(len(run_df)), 'window_bytes': a.window_bytes, 'write_s': round(write_s, 1),
                          'read_s': round(t['read_s'], 3), 'copy_in_ms': round(t['copy_ms'], 1),
                          'scan_device_ms': round(t['device_ms'], 2),
                          'scan_gbps': round(size / (t['device_ms'] * 1e-3) / 1e9, 1) if t['device_ms'] > 0 else None,
                          'hbm_peak_gbps': HBM_PEAK_GBPS, 'hbm_copy_gbps': HBM_COPY_GBPS,
                          'get_data_s': round(get_data_s, 2), 'run_s': round(run_s, 2)}))
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

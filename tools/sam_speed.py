"""
Speed of the SAM path (degnorm_amd.bam.sam_to_bam; csrc/dn_sam.hip) on the 2 M-read single-end file of tools/bam_speed.py
(tests/_reads_fixtures.scale_case: 20 Mb, 2 M reads of the forms aM / aMnNbM), written as SAM text with the optional fields
of the test fixtures (tests/_sam_cases.sam_text), in input (shuffled) order.  One JSON line per mode:

  device0 / host    sam_to_bam with device=0 and with device=None (the host build of the same source), alternated in one
                    process, --reps repetitions each behind one unmeasured pass; every figure as [minimum, maximum]
  read_ms           reading the file and cutting it into windows
  copy_ms           the copy of the text to the device, by events (0 on the host)
  encode_device_ms  first kernel to last of every window, by events (0 on the host); text_gbps: text bytes over it, next to
                    read_gbps, the read ceiling dn_measure_read_gbps reports in the same process
  encode_ms         the encode calls as the host sees them (allocation, copies in and out, kernels, the strtod patches)
  deflate_ms        deflating the blocks (zlib in --jobs threads, or --deflate native on the same device)
  e2e_ms            the whole conversion, file to file

    python tools/sam_speed.py [--reads 2000000] [--jobs 16] [--reps 3] [--dir DIR] [--deflate zlib|native] [--limit 300]

Every conversion runs under --limit seconds (SIGALRM): a step that takes longer ends the program with an error instead of
being waited for.  Files found in --dir from an earlier run with the same --reads are used again.  Needs a GPU.
"""
import argparse
import json
import os
import shutil
import signal
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                                   # noqa: E402
import pandas as pd                                  # noqa: E402

import _reads_fixtures as rf                         # noqa: E402
import _sam_cases as sc                              # noqa: E402
from degnorm_amd import _lib, bam                    # noqa: E402


def _timed_out(signum, frame):
    raise TimeoutError('a step of sam_speed ran beyond its time limit')


def _limited(limit, call):
    signal.signal(signal.SIGALRM, _timed_out)
    signal.alarm(int(limit))
    try:
        return call()
    finally:
        signal.alarm(0)


def _convert(src, dst, device, jobs, deflate):
    stats = {}
    t0 = time.perf_counter()
    bam.sam_to_bam(src, dst, device=device, n_jobs=jobs, deflate=deflate, overwrite=True, stats=stats)
    e2e = time.perf_counter() - t0
    return {'read_ms': 1e3 * stats['read_s'], 'copy_ms': stats['copy_ms'], 'encode_device_ms': stats['encode_device_ms'],
            'encode_ms': 1e3 * stats['encode_s'], 'deflate_ms': 1e3 * stats['deflate_s'], 'e2e_ms': 1e3 * e2e}, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=2_000_000)
    ap.add_argument('--jobs', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--dir', default=None)
    ap.add_argument('--deflate', choices=['zlib', 'native'], default='zlib')
    ap.add_argument('--limit', type=int, default=300, help='seconds a single conversion may take')
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix='sam_speed_')
    try:
        os.makedirs(work, exist_ok=True)
        src = os.path.join(work, 'se_{0}.sam'.format(a.reads))
        t0 = time.perf_counter()
        if not os.path.isfile(src):
            reads, chrom_len, _, _, _ = rf.scale_case(n_reads=a.reads)
            rows = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values,
                                 'nh': 1, 'nh_type': 'C'})
            rows = rows.iloc[np.random.default_rng(1).permutation(len(rows))].reset_index(drop=True)
            refs = [('chrS', chrom_len)]
            sc.write_sam(src, sc.sam_text(rows, refs), '@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrS\tLN:{0}\n'.format(chrom_len))
        write_s = time.perf_counter() - t0
        dev = _lib.Device(0)
        read_gbps = dev.measure_read_gbps(1 << 30, 5)
        dev.close()
        modes = {'device0': 0, 'host': None}
        rows_of = {m: [] for m in modes}
        files = {m: os.path.join(work, 'out_{0}.bam'.format(m)) for m in modes}
        last = {}
        for k in range(a.reps + 1):                      # the first pass loads the library and warms the device up
            for m, device in modes.items():
                row, last[m] = _limited(a.limit, lambda: _convert(src, files[m], device, a.jobs, a.deflate))
                if k > 0:
                    rows_of[m].append(row)
        same = open(files['device0'], 'rb').read() == open(files['host'], 'rb').read()
        text_bytes = os.path.getsize(src)
        for m in modes:
            out = {'tool': 'sam_speed', 'mode': m, 'reads': a.reads, 'jobs': a.jobs, 'deflate': a.deflate, 'reps': a.reps,
                   'sam_mb': round(text_bytes / 2 ** 20, 1), 'bam_mb': round(last[m]['bytes_out'] / 2 ** 20, 1),
                   'record_mb': round(last[m]['record_bytes'] / 2 ** 20, 1), 'windows': last[m]['windows'], 'records': last[m]['records'],
                   'float_patches': last[m]['float_patches'], 'write_s': round(write_s, 1), 'same_file_as_other_mode': same}
            for key in ('read_ms', 'copy_ms', 'encode_device_ms', 'encode_ms', 'deflate_ms', 'e2e_ms'):
                vals = [r[key] for r in rows_of[m]]
                out[key] = [round(min(vals), 3), round(max(vals), 3)]
            if m == 'device0':
                ms = out['encode_device_ms']
                out['text_gbps'] = [round(text_bytes / (ms[1] * 1e-3) / 1e9, 2), round(text_bytes / (ms[0] * 1e-3) / 1e9, 2)]
                out['read_gbps'] = round(read_gbps, 1)
            out['reads_per_s'] = round(a.reads / (out['e2e_ms'][0] * 1e-3))
            print(json.dumps(out))
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

"""
Speed of .bai creation (degnorm_amd.bam.create_index) on the 2 M-read single-end file of tools/bam_speed.py, written without
an index at deflate levels 1 and 6:

  device     create_index(device=0) end to end (blocks read, uploaded, inflated, framed and indexed on the GPU, tables
             stitched, file written), and the split the library reports: inflate_device_ms, frame_device_ms, index_device_ms
             (by events), frame_fixups, records, chunks, windows
  host       create_index(device=None, n_jobs=--jobs): zlib in a thread pool and the host build of the same source

The two modes run alternated, --reps times each after one warm-up each; every figure is reported as [minimum, maximum] over
the repetitions.  `same` says whether the two wrote the same bytes.  When a samtools is on PATH, `samtools index -@ 16` is
timed on the same file and its output compared with ours (`samtools_same`); otherwise samtools is "not compared with
samtools".  Nothing is fetched.  --format csi times the .csi index instead (min_shift 14, the depth left to the library;
its file is BGZF-compressed on the host, which e2e_ms includes); samtools is then not run.

    python tools/bai_speed.py [--reads 2000000] [--jobs 16] [--reps 3] [--levels 1,6] [--modes device,host] [--dir DIR]
                              [--format bai|csi]

Prints one JSON line.  Needs a GPU unless --modes host.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pandas as pd                                  # noqa: E402

import _bam_fixtures as bf                           # noqa: E402
import _reads_fixtures as rf                         # noqa: E402
from degnorm_amd import bam                          # noqa: E402

SPLIT = ('inflate_device_ms', 'frame_device_ms', 'index_device_ms')


def _span(values, digits=1):
    return [round(min(values), digits), round(max(values), digits)]


def _level(path, modes, jobs, reps, verify=False, fmt='bai'):
    rows = {m: [] for m in modes}
    out = {}
    for k in range(reps + 1):                        # the first round loads the library and warms the device up
        for m in modes:
            stats = {}
            t0 = time.perf_counter()
            bam.create_index(path, path + '.' + m, overwrite=True, device=0 if m == 'device' else None, n_jobs=jobs, stats=stats, verify=verify,
                             fmt=fmt)
            stats['e2e_ms'] = 1e3 * (time.perf_counter() - t0)
            if k > 0:
                rows[m].append(stats)
    for m in modes:
        out[m] = {'e2e_ms': _span([r['e2e_ms'] for r in rows[m]])}
        if m == 'device':
            out[m].update({key: _span([r[key] for r in rows[m]], 3) for key in SPLIT})
        out[m].update({key: rows[m][-1][key] for key in ('frame_fixups', 'records', 'chunks', 'windows')})
    if len(modes) == 2:
        with open(path + '.' + modes[0], 'rb') as fa, open(path + '.' + modes[1], 'rb') as fb:
            out['same'] = fa.read() == fb.read()
    out['bai_bytes'] = os.path.getsize(path + '.' + modes[0])
    samtools = shutil.which('samtools') if fmt == 'bai' else None
    if samtools is None:
        out['samtools'] = 'not compared with samtools'
    else:
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run([samtools, 'index', '-@', '16', path, path + '.samtools'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            times.append(1e3 * (time.perf_counter() - t0))
        out['samtools'] = {'e2e_ms': _span(times), 'returncode': r.returncode}
        if r.returncode == 0:
            with open(path + '.samtools', 'rb') as fa, open(path + '.' + modes[0], 'rb') as fb:
                out['samtools_same'] = fa.read() == fb.read()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=2_000_000)
    ap.add_argument('--jobs', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--levels', default='1,6')
    ap.add_argument('--modes', default='device,host')
    ap.add_argument('--dir', default=None)
    ap.add_argument('--format', choices=('bai', 'csi'), default='bai', help='the index format to time')
    ap.add_argument('--verify', action='store_true', help='check every BGZF block against the CRC32 of its trailer')
    a = ap.parse_args()
    modes = [m for m in ('device', 'host') if m in a.modes.split(',')]
    reads, chrom_len, _, _, _ = rf.scale_case(n_reads=a.reads)
    se = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
    work = a.dir or tempfile.mkdtemp(prefix='bai_speed_')
    try:
        os.makedirs(work, exist_ok=True)
        out = {'tool': 'bai_speed', 'reads': a.reads, 'jobs': a.jobs, 'reps': a.reps, 'modes': modes}
        if a.verify:
            out['verify'] = True
        if a.format != 'bai':
            out['format'] = a.format
        for level in (int(x) for x in a.levels.split(',')):
            path = os.path.join(work, 'se_{0}_l{1}.bam'.format(a.reads, level))
            if not os.path.isfile(path):
                bf.write_bam(path, [('chrS', chrom_len)], se, level=level, index=False)
            row = _level(path, modes, a.jobs, a.reps, a.verify, a.format)
            row['bam_mb'] = round(os.path.getsize(path) / 2 ** 20, 1)
            row['inflated_mb'] = round(int(bam.bgzf_blocks(path)[2].sum()) / 2 ** 20, 1)
            out['level{0}'.format(level)] = row
        print(json.dumps(out))
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

"""
Speed of the coordinate sort of a BAM file (degnorm_amd.bam.sort_bam) on the 2 M-read single-end file of tools/bam_speed.py
with its records permuted by a seed and its header saying SO:unsorted:

  device     sort_bam(device=0, n_jobs=--jobs) end to end (blocks read, uploaded, inflated, framed, keyed, sorted and gathered
             on the GPU, the sorted stream fetched, deflated by zlib in --jobs threads and written), and the split the library
             reports: inflate_device_ms, frame_device_ms, sort_device_ms, gather_device_ms (by events), deflate_s
  host       sort_bam(device=None, n_jobs=--jobs): zlib inflate in the same pool and the host build of the same source

--deflate native has the blocks written by the library's own encoder (csrc/dn_deflate.hip) in place of zlib: on the device the
sorted stream is deflated where it lies and only the blocks are fetched.  Every line then also holds deflate_device_ms (the
encoder's kernels, by events), out_bytes (the blocks that hold records), out_file_bytes (the size of the written file) and,
for the device, fetched_bytes: what came back from the device after the sort -- the record ends and the sorted stream ('zlib')
or the blocks ('native').

The two modes run alternated in one process, --reps times each after one warm-up each; every figure is reported as [minimum,
maximum] over the repetitions.  `same` says whether the two wrote the same bytes.  The device line also holds the yardstick
of the gather kernel: a device-to-device hipMemcpyAsync of the same byte count, timed by events in this
process, both as bytes read + bytes written per second.

    python tools/sort_speed.py [--reads 2000000] [--jobs 16] [--reps 5] [--level 1] [--seed 0] [--modes device,host] [--deflate zlib]
                                [--dir DIR]

Prints one JSON line per mode.  Needs a GPU unless --modes host.
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

SPLIT = ('inflate_device_ms', 'frame_device_ms', 'sort_device_ms', 'gather_device_ms')


def _span(values, digits=1):
    return [round(min(values), digits), round(max(values), digits)]


def write_permuted(path, refs, rows, seed, level):
    """The rows' records (encoded in sorted order, as tools/bam_speed.py's file holds them) written in a seeded order."""
    data, offs = bf.encode_records(bf.sort_reads(rows))
    ends = np.append(offs[1:], len(data))
    order = np.random.default_rng(seed).permutation(len(offs))
    view = memoryview(data)
    stream = b''.join([view[a:b] for a, b in zip(offs[order].tolist(), ends[order].tolist())])
    with open(path, 'wb') as f:
        f.write(bf._bgzf_block(bf.header_bytes(refs, text='@HD\tVN:1.6\tSO:unsorted\n'), level))
        for a in range(0, len(stream), 0xff00):
            f.write(bf._bgzf_block(stream[a:a + 0xff00], level))
        f.write(bf.EOF_BLOCK)
    return len(stream)


def d2d_copy_ms(n_bytes, reps, device=0):
    """ms of each of `reps` hipMemcpyAsync device-to-device copies of n_bytes, by events, after one warm-up.  The HIP runtime
    is the one the library is linked to, reached through the library's own handle."""
    import ctypes
    from degnorm_amd import _lib
    hip = ctypes.CDLL(_lib.LIB_PATH)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError('{0} failed with HIP error {1}'.format(what, rc))

    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    hip.hipMemset.argtypes = [vp, ctypes.c_int, sz]
    hip.hipMemcpyAsync.argtypes = [vp, vp, sz, ctypes.c_int, vp]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    hip.hipFree.argtypes = [vp]
    ok(hip.hipSetDevice(int(device)), 'hipSetDevice')
    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    times = []
    try:
        ok(hip.hipMalloc(ctypes.byref(src), n_bytes), 'hipMalloc')
        ok(hip.hipMalloc(ctypes.byref(dst), n_bytes), 'hipMalloc')
        ok(hip.hipMemset(src, 0, n_bytes), 'hipMemset')
        ok(hip.hipEventCreate(ctypes.byref(e0)), 'hipEventCreate')
        ok(hip.hipEventCreate(ctypes.byref(e1)), 'hipEventCreate')
        for k in range(reps + 1):
            ms = ctypes.c_float(0.0)
            ok(hip.hipEventRecord(e0, None), 'hipEventRecord')
            ok(hip.hipMemcpyAsync(dst, src, n_bytes, 3, None), 'hipMemcpyAsync')          # 3: hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(e1, None), 'hipEventRecord')
            ok(hip.hipEventSynchronize(e1), 'hipEventSynchronize')
            ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), 'hipEventElapsedTime')
            if k > 0:
                times.append(float(ms.value))
    finally:
        for e in (e0, e1):
            if e:
                hip.hipEventDestroy(e)
        for b in (src, dst):
            if b:
                hip.hipFree(b)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=2_000_000)
    ap.add_argument('--jobs', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--level', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--modes', default='device,host')
    ap.add_argument('--deflate', choices=('zlib', 'native'), default='zlib')
    ap.add_argument('--dir', default=None)
    a = ap.parse_args()
    modes = [m for m in ('device', 'host') if m in a.modes.split(',')]
    reads, chrom_len, _, _, _ = rf.scale_case(n_reads=a.reads)
    se = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
    work = a.dir or tempfile.mkdtemp(prefix='sort_speed_')
    try:
        os.makedirs(work, exist_ok=True)
        path = os.path.join(work, 'se_{0}_l{1}_seed{2}.bam'.format(a.reads, a.level, a.seed))
        if not os.path.isfile(path):
            write_permuted(path, [('chrS', chrom_len)], se, a.seed, a.level)
        n_stream = int(bam.bgzf_blocks(path)[2].sum())
        rows = {m: [] for m in modes}
        for k in range(a.reps + 1):                  # the first round loads the library and warms the device up
            for m in modes:
                stats = {}
                t0 = time.perf_counter()
                bam.sort_bam(path, path + '.' + m, overwrite=True, device=0 if m == 'device' else None, n_jobs=a.jobs, level=a.level, stats=stats,
                             deflate=a.deflate)
                stats['e2e_ms'] = 1e3 * (time.perf_counter() - t0)
                if k > 0:
                    rows[m].append(stats)
        same = None
        if len(modes) == 2:
            with open(path + '.' + modes[0], 'rb') as fa, open(path + '.' + modes[1], 'rb') as fb:
                same = fa.read() == fb.read()
        for m in modes:
            out = {'tool': 'sort_speed', 'mode': m, 'reads': a.reads, 'jobs': a.jobs, 'reps': a.reps, 'level': a.level, 'seed': a.seed,
                   'bam_mb': round(os.path.getsize(path) / 2 ** 20, 1), 'inflated_mb': round(n_stream / 2 ** 20, 1),
                   'sorted_order': bam.sort_order(path + '.' + m), 'e2e_ms': _span([r['e2e_ms'] for r in rows[m]]),
                   'deflate_s': _span([r['deflate_s'] for r in rows[m]], 3), 'deflate': a.deflate,
                   'deflate_device_ms': _span([r['deflate_device_ms'] for r in rows[m]], 3), 'out_bytes': rows[m][-1]['out_bytes'],
                   'out_file_bytes': os.path.getsize(path + '.' + m)}
            out.update({key: rows[m][-1][key] for key in ('records', 'bytes', 'windows', 'frame_fixups')})
            if same is not None:
                out['same'] = same
            if m == 'device':
                out['fetched_bytes'] = 8 * rows[m][-1]['records'] + rows[m][-1]['bytes' if a.deflate == 'zlib' else 'out_bytes']
                out.update({key: _span([r[key] for r in rows[m]], 3) for key in SPLIT})
                n = rows[m][-1]['bytes']
                copy = d2d_copy_ms(n, a.reps)
                out['d2d_copy_ms'] = _span(copy, 3)
                out['gather_gbps'] = _span([2e-6 * n / r['gather_device_ms'] for r in rows[m]])
                out['d2d_copy_gbps'] = _span([2e-6 * n / t for t in copy])
            print(json.dumps(out))
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

"""
Speed of the gzip inflate (degnorm_amd.gz.gunzip with device=0) against one zlib thread -- what gzip.open, and so every other
reader of a .gtf.gz, does -- on the seeded GENCODE-style GTF of tests/_gtf_fixtures.write_gtf, gzip'd at level 6.  The two are
alternated in one process: after a warm-up of each, --reps repetitions, minimum and maximum of each.  One JSON line: the sizes,
the two ranges, the stage times (HIP events) and counters of the fastest device repetition, and the counters at 16, 64 and 256
KiB chunks.

    python tools/gz_speed.py [--bytes 419430400] [--reps 5] [--chunk-bytes 65536] [--dir DIR]

Needs a GPU.  The default text is a 400 MB cut of the 1.5 GB that tools/gtf_speed.py writes: the generator and level-6 zlib
take most of a minute per 400 MB.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _gtf_fixtures as gf                           # noqa: E402
from degnorm_amd import gz                           # noqa: E402

KEEP = ('members', 'chunks', 'guessed', 'confirmed', 'jumped', 'fixups', 'segments', 'blocks')


def zlib_thread(data):
    """The inflated size by one zlib.decompressobj, fed and drained in 1 MiB pieces as gzip.open does."""
    d, n = zlib.decompressobj(31), 0
    for lo in range(0, len(data), 1 << 20):
        n += len(d.decompress(data[lo:lo + (1 << 20)]))
    return n + len(d.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=400 << 20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chunk-bytes', type=int, default=gz.CHUNK_BYTES)
    ap.add_argument('--dir', default=None)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix='gz_speed_')
    try:
        path = os.path.join(work, 'seeded.gtf')
        t0 = time.perf_counter()
        _, _, size = gf.write_gtf(path, 7, a.bytes)
        with open(path, 'rb') as f:
            text = f.read()
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        data = co.compress(text) + co.flush()
        make_s = time.perf_counter() - t0
        assert gz.gunzip(data, device=0, chunk_bytes=a.chunk_bytes) == text and zlib_thread(data) == size      # warm-up, and the bytes
        del text
        dev, ref, best = [], [], None
        for _ in range(a.reps):
            st = {}
            t0 = time.perf_counter()
            n = len(gz.gunzip(data, device=0, chunk_bytes=a.chunk_bytes, stats=st))
            dev.append(time.perf_counter() - t0)
            assert n == size
            if dev[-1] == min(dev):
                best = st
            t0 = time.perf_counter()
            assert zlib_thread(data) == size
            ref.append(time.perf_counter() - t0)
        by_chunk = {}
        for kib in (16, 64, 256):
            st = {}
            t0 = time.perf_counter()
            gz.gunzip(data, device=0, chunk_bytes=kib << 10, stats=st)
            by_chunk[str(kib)] = dict({k: st[k] for k in ('guessed', 'confirmed', 'fixups', 'segments')}, s=round(time.perf_counter() - t0, 3),
                                      device_ms=round(sum(st[k] for k in gz.STAGES), 1))
        print(json.dumps({'tool': 'gz_speed', 'text_bytes': size, 'gz_bytes': len(data), 'level': 6, 'chunk_bytes': a.chunk_bytes, 'reps': a.reps,
                          'make_s': round(make_s, 1),
                          'device_s': [round(min(dev), 3), round(max(dev), 3)], 'zlib_thread_s': [round(min(ref), 3), round(max(ref), 3)],
                          'device_gbps_out': round(size / min(dev) / 1e9, 2), 'zlib_gbps_out': round(size / min(ref) / 1e9, 2),
                          'stages_ms': {k: round(best[k], 2) for k in gz.STAGES}, 'counters': {k: best[k] for k in KEEP},
                          'by_chunk_kib': by_chunk}))
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

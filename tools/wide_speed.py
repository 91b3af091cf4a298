"""Wide cohorts (65 .. 256 samples, kernel family gen_wide): GeneNMFOA.run() on seeded synthetic cohorts, plain and with take-every
500, one JSON line per (p, regime): the stage timings of run(), the device time of the initial pass and of each iteration kernel,
genes per second, the bytes of coverage the initial pass streams per second.  p <= 64 runs the same on the existing families
(the comparison point); --oracle-head N times the CPU oracle's run on the first N genes with 16 threads.
usage (GPU box): python tools/wide_speed.py [--genes 2000] [--lmin 200] [--lmax 3000] [--iters 2] [--oracle-head 0] [p ...]"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from degnorm_amd import synth
from degnorm_amd.nmf import GeneNMFOA

ap = argparse.ArgumentParser()
ap.add_argument('p', nargs='*', type=int, default=[96, 128, 256])
ap.add_argument('--genes', type=int, default=2000)
ap.add_argument('--lmin', type=int, default=600)           # longer than the take-every rate
ap.add_argument('--lmax', type=int, default=3000)
ap.add_argument('--iters', type=int, default=2)
ap.add_argument('--nmf-iter', type=int, default=100)
ap.add_argument('--oracle-head', type=int, default=0)
args = ap.parse_args()

for p in args.p:
    packed, lengths, reads, _ = synth.synth_packed(96, range(args.genes), p, args.lmin, args.lmax, n_threads=16)
    offs = np.concatenate([[0], np.cumsum(lengths * p)])
    cov = OrderedDict(('gene_%06d' % g, packed[offs[g]:offs[g + 1]].reshape(p, int(lengths[g]))) for g in range(args.genes))
    for rate in (1, 500):
        m = GeneNMFOA(degnorm_iter=args.iters, nmf_iter=args.nmf_iter, downsample_rate=rate, random_state=1)
        t0 = time.perf_counter()
        m.run(cov, reads)
        wall = time.perf_counter() - t0
        dev = m._dev
        init_ms = dev.last_init_ms()
        out = dict(p=p, regime='plain' if rate == 1 else 'take-every-%d' % rate, genes=args.genes, bases=int(lengths.sum()),
                   degnorm_iter=args.iters, nmf_iter=args.nmf_iter, wall_s=round(wall, 4),
                   timings={k: round(v, 4) for k, v in m.timings.items()},
                   init_kernel=dev.init_kernel_name(), init_ms=round(init_ms, 3),
                   init_cov_gbps=round(4.0 * p * float(lengths.sum()) / (init_ms * 1e-3) / 1e9, 1) if init_ms > 0 else None,
                   iter_kernel=dev.class_kernel_name(0), iter_ms=[round(float(v), 3) for v in m.kernel_ms],
                   genes_per_s_run=round(args.genes / m.timings['run_s'], 1),
                   genes_per_s_iter_kernel=round(args.genes / (min(m.kernel_ms) * 1e-3), 1) if len(m.kernel_ms) else None,
                   status_nonzero=int(sum(int((tr[:, 6] != 0).sum()) for tr in m.traces)))
        if args.oracle_head > 0 and rate == 1:
            from oracle import oracle
            oracle.build()
            head = list(cov.values())[:args.oracle_head]
            t0 = time.perf_counter()
            oracle.run([np.asarray(c, dtype=np.float64) for c in head], reads[:args.oracle_head], degnorm_iter=args.iters,
                       nmf_iter=args.nmf_iter, n_threads=16)
            dt = time.perf_counter() - t0
            out['oracle_head'] = args.oracle_head
            out['oracle_genes_per_s_16_threads'] = round(args.oracle_head / dt, 2)
        print(json.dumps(out), flush=True)
        dev.close()

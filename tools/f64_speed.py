"""
Device time of the float64-input path next to the CPU oracle on this host's cores:

  nmf      10 000 matrices of 10 x 1 000 at T = 100, one dn_nmf_f64 call (oracle: one thread on a slice, scaled up)
  ratio    the same batch through ratio_svd (dn_nmf_f64 DN_NMF_RATIO; oracle: ratio_svd_batch on all cores)
  genes    the 72 genes of tests/golden/genes.npz scaled by 1/s, one dn_baseline_selection_f64 call with estimates
           (oracle: baseline_batch on all cores)

    python tools/f64_speed.py [--matrices 10000] [--oracle-slice 100]

Prints one JSON line.  Needs a GPU; the oracle is test infrastructure (oracle/), used here only as the yardstick.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                                   # noqa: E402

from degnorm_amd import _lib, synth                  # noqa: E402
from oracle import oracle as orc                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--matrices', type=int, default=10000)
    ap.add_argument('--oracle-slice', type=int, default=100)
    a = ap.parse_args()
    orc.build()
    dev = _lib.Device(0)
    rng = np.random.RandomState(0)
    mats = [np.outer(rng.lognormal(size=10), rng.lognormal(size=1000)) * rng.lognormal(0.0, 0.4, size=(10, 1000))
            for _ in range(a.matrices)]
    out = {'host_cores': os.cpu_count(), 'matrices': a.matrices}

    dev.nmf_f64(mats[:64], _lib.NMF, 100)                                     # warm-up (code object load)
    t = time.perf_counter()
    _, _, _, st = dev.nmf_f64(mats, _lib.NMF, 100)
    wall = time.perf_counter() - t
    k = min(a.oracle_slice, len(mats))
    t = time.perf_counter()
    for x in mats[:k]:
        orc.nmf(x, 100)
    o1 = (time.perf_counter() - t) * len(mats) / k
    out['nmf_T100'] = dict(device_ms=dev.last_f64_ms(), call_wall_s=wall, failed=int((st != 0).sum()),
                           oracle_1thread_s=o1, oracle_all_cores_s_est=o1 / os.cpu_count())

    t = time.perf_counter()
    _, _, _, st = dev.nmf_f64(mats, _lib.NMF_RATIO, 0, want_est=True)
    wall = time.perf_counter() - t
    t = time.perf_counter()
    orc.ratio_svd_batch(mats, n_threads=0)
    out['ratio_svd'] = dict(device_ms=dev.last_f64_ms(), call_wall_s=wall, failed=int((st != 0).sum()),
                            oracle_all_cores_s=time.perf_counter() - t)

    G = np.load(os.path.join(ROOT, 'tests', 'golden', 'genes.npz'))
    p = int(G['p'])
    covs = [synth.synth_gene(int(G['seed']), int(g), p, int(G['l_min']), int(G['l_max']))[0] for g in G['gene_ids']]
    F = [c / G['scale'][:, None] for c in covs]
    dev.baseline_selection_f64(F, nmf_iter=int(G['nmf_iter']), want_est=True)
    t = time.perf_counter()
    rho, _, trace, _ = dev.baseline_selection_f64(F, nmf_iter=int(G['nmf_iter']), want_est=True)
    wall = time.perf_counter() - t
    t = time.perf_counter()
    orc.baseline_batch(covs, G['scale'], orc.make_params(nmf_iter=int(G['nmf_iter'])), want_estimates=True, n_threads=0)
    out['genes72'] = dict(device_ms=dev.last_f64_ms(), call_wall_s=wall, failed=int((trace[:, 6] != 0).sum()),
                          max_rel_err_rho=float(np.max(np.abs(rho - G['rho']) / np.maximum(np.abs(G['rho']), 1e-11))),
                          oracle_all_cores_s=time.perf_counter() - t)
    dev.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()

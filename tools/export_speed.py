"""
Speed of the coverage export (degnorm_amd.data_access.get_coverage_data; csrc/dn_text.hip) against the reference's writer.
--genes seeded genes (2 000) of 600 to 3 000 bases at p = 10 -- raw counts from degnorm_amd.synth, estimates of arbitrary
float64 -- are written once as an output directory on 20 chromosomes; get_coverage_data('all', dir, save_dir) is then timed
with formatter='device' and formatter='pandas' (the reference's to_csv call), alternated in one process, --reps repetitions
each.  Before them both formatters run once, unmeasured, on the first --warmup-genes genes: that loads the libraries, opens
the device and touches the directory.  One JSON line, with the figures of each formatter under its name as [minimum, maximum]:

  e2e_s            the whole call, directory to files
  load_s           reading the .csv files and the pickles (the same code for both)
  format_call_s    (device) the dn_cov_text calls as the host sees them: packing the matrices, allocation, copies, kernels
  upload_ms, measure_ms, scan_ms, emit_ms, copy_back_ms   (device) by HIP events, summed over the batches
  write_s          (device) writing the files from the pinned text in --jobs threads
  pandas_s         the to_csv calls (all files with 'pandas'; with 'device' only the flagged ones, here none)
  values_per_s     matrix entries over the slowest e2e_s
  emit_gbps        text bytes over emit_ms, next to read_gbps, the read ceiling dn_measure_read_gbps reports in this process
  same_files       whether the two formatters left the same bytes in every file
  device_wins      whether the slowest 'device' repetition end to end lies below the fastest 'pandas' one

    python tools/export_speed.py [--genes 2000] [--reps 3] [--jobs 1] [--warmup-genes 50] [--dir DIR] [--limit 600]

Every call runs under --limit seconds (SIGALRM): one that takes longer ends the program with an error instead of being
waited for.  Needs a GPU.
"""
import argparse
import hashlib
import json
import os
import pickle
import shutil
import signal
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                   # noqa: E402
from pandas import DataFrame                         # noqa: E402

from degnorm_amd import _lib, data_access as da, synth       # noqa: E402

P, L_MIN, L_MAX, SEED, N_CHROM = 10, 600, 3000, 41, 20


def _timed_out(signum, frame):
    raise TimeoutError('a step of export_speed ran beyond its time limit')


def _limited(limit, call):
    signal.signal(signal.SIGALRM, _timed_out)
    signal.alarm(int(limit))
    try:
        return call()
    finally:
        signal.alarm(0)


def write_directory(path, n_genes):
    rng = np.random.default_rng(SEED)
    samples = ['sample_{0}'.format(k + 1) for k in range(P)]
    raw = {'chr{0}'.format(c + 1): {} for c in range(N_CHROM)}
    est = {c: {} for c in raw}
    rows, values = [], 0
    for g in range(n_genes):
        chrom, gene = 'chr{0}'.format(g % N_CHROM + 1), 'GENE{0}'.format(g)
        cov = synth.synth_gene(SEED, g, P, L_MIN, L_MAX)[0]
        raw[chrom][gene] = cov
        est[chrom][gene] = cov * rng.uniform(0.3, 3.0, size=(P, 1)) * rng.uniform(0.9, 1.1, size=cov.shape) + rng.uniform(0, 1e-3, size=cov.shape)
        rows.append((chrom, 1000 + 10000 * g, 1000 + 10000 * g + cov.shape[1], gene, g, 1000 + 10000 * g + cov.shape[1], 1000 + 10000 * g))
        values += 2 * cov.size
    os.makedirs(path)
    DataFrame(rows, columns=['chr', 'start', 'end', 'gene', 'exon_id', 'gene_end', 'gene_start']).to_csv(os.path.join(path, 'gene_exon_metadata.csv'),
                                                                                                           index=False)
    di = DataFrame({'chr': [r[0] for r in rows], 'gene': [r[3] for r in rows]})
    for s in samples:
        di[s] = 0.25
    di.to_csv(os.path.join(path, 'degradation_index_scores.csv'), index=False)
    di.to_csv(os.path.join(path, 'read_counts.csv'), index=False)
    for chrom in raw:
        os.makedirs(os.path.join(path, chrom))
        with open(os.path.join(path, chrom, 'coverage_matrices_{0}.pkl'.format(chrom)), 'wb') as f:
            pickle.dump(raw[chrom], f)
        with open(os.path.join(path, chrom, 'estimated_coverage_matrices_{0}.pkl'.format(chrom)), 'wb') as f:
            pickle.dump(est[chrom], f)
    return values


def tree_digest(root):
    h, n = hashlib.sha256(), 0
    for d, dirs, names in os.walk(root):
        dirs.sort()
        for name in sorted(names):
            h.update(os.path.relpath(os.path.join(d, name), root).encode())
            with open(os.path.join(d, name), 'rb') as f:
                h.update(f.read())
            n += 1
    return h.hexdigest(), n


def export(genes, src, dst, formatter, jobs):
    shutil.rmtree(dst, ignore_errors=True)
    stats = {}
    t0 = time.perf_counter()
    da.get_coverage_data(genes, src, save_dir=dst, device=0, n_jobs=jobs, formatter=formatter, stats=stats)
    stats['e2e'] = time.perf_counter() - t0
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--jobs', type=int, default=1)
    ap.add_argument('--warmup-genes', type=int, default=50)
    ap.add_argument('--dir', default=None)
    ap.add_argument('--limit', type=int, default=600, help='seconds a single call may take')
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix='export_speed_')
    try:
        src = os.path.join(work, 'degnorm_out')
        shutil.rmtree(src, ignore_errors=True)
        t0 = time.perf_counter()
        values = write_directory(src, a.genes)
        setup_s = time.perf_counter() - t0
        dev = _lib.Device(0)
        read_gbps = dev.measure_read_gbps(1 << 30, 5)
        dev.close()
        modes = ('device', 'pandas')
        dst = {m: os.path.join(work, 'saved_' + m) for m in modes}
        warm = ['GENE{0}'.format(g) for g in range(min(a.warmup_genes, a.genes))]
        for m in modes:
            _limited(a.limit, lambda: export(warm, src, dst[m], m, a.jobs))
        runs = {m: [] for m in modes}
        for _ in range(a.reps):
            for m in modes:
                runs[m].append(_limited(a.limit, lambda: export('all', src, dst[m], m, a.jobs)))
                print('{0}: {1:.2f} s'.format(m, runs[m][-1]['e2e']), file=sys.stderr, flush=True)
        digests = {m: tree_digest(dst[m]) for m in modes}
        slow_device, fast_pandas = max(r['e2e'] for r in runs['device']), min(r['e2e'] for r in runs['pandas'])
        line = {'tool': 'export_speed', 'genes': a.genes, 'p': P, 'values': values, 'files': digests['device'][1], 'jobs': a.jobs, 'reps': a.reps,
                'setup_s': round(setup_s, 1), 'same_files': digests['device'] == digests['pandas'], 'read_gbps': round(read_gbps, 1),
                'device_wins': slow_device < fast_pandas}
        for m in modes:
            out = {}
            assert all(r['values'] == values for r in runs[m])
            for key, name in (('e2e', 'e2e_s'), ('load', 'load_s'), ('format_call', 'format_call_s'), ('write', 'write_s'), ('pandas', 'pandas_s')):
                vals = [r[key] for r in runs[m]]
                out[name] = [round(min(vals), 3), round(max(vals), 3)]
            out['values_per_s'] = round(values / out['e2e_s'][1])
            if m == 'device':
                for key in ('upload_ms', 'measure_ms', 'scan_ms', 'emit_ms', 'copy_back_ms'):
                    vals = [r[key] for r in runs[m]]
                    out[key] = [round(min(vals), 3), round(max(vals), 3)]
                text_bytes = runs[m][0]['text_bytes']
                out.update(text_mb=round(text_bytes / 2 ** 20, 1), batches=runs[m][0]['batches'], flagged_files=runs[m][0]['flagged_files'],
                           emit_gbps=[round(text_bytes / (out['emit_ms'][1] * 1e-3) / 1e9, 2), round(text_bytes / (out['emit_ms'][0] * 1e-3) / 1e9, 2)])
            line[m] = out
        print(json.dumps(line), flush=True)
    finally:
        if a.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()

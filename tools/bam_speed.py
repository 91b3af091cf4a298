"""
Speed of the native BAM path (degnorm_amd.bam.NativeBamReadsProcessor) on the synthetic scale chromosome of the GPU tests
(tests/_reads_fixtures.scale_case: 20 Mb, 2 000 genes, 2 M single-end reads of the forms aM / aMnNbM), written as a sorted,
indexed BAM, and on a paired variant (the same reads named <i // 2>.1 / .2, mates next to each other; with --pairing flag
both mates are named <i // 2> and carry FLAG 0x41 / 0x81 plus strand bits and the mate's position as PNEXT, as an aligner
writes them, and the reader pairs them by FLAG):

  inflate_ms        BGZF inflate of the chromosome's blocks: zlib on the host in n_jobs threads (--inflate host), or the
                    library's DEFLATE kernel with the copy of the compressed blocks in and of the window back (--inflate device)
  inflate_device_ms the DEFLATE kernel alone, by events (0 with --inflate host); inflate_gbps: inflated bytes over it
  frame_ms          host record framing (dn_bam_frame; 0 with --frame device)
  frame_device_ms   record framing on the device (--frame device): first framing kernel to the last of every window, by events,
                    the host's stitch of the segment table between them included; frame_fixups: segments walked again
  decode_ms         the append calls: window upload, decode / filter kernels, compaction into the row store (with --frame
                    device the library's own clock around decode and compaction; the upload of a host-inflated window is
                    upload_ms then)
  coverage_ms       the coverage call on the stored rows (paired: with the key download and the host sort, or with
                    --pair device the pairing on the device)
  pair_device_ms    the pairing on the device alone, by events (0 with --pair host and for single-end)
  coverage_device_ms  device time of the coverage stages (events on its stream)
  reads_per_s       end to end: reads / chromosome_coverage_read_counts (files written, index and header already read)
  in_memory_reads_per_s  chromosome_coverage_read_counts_df on the same reads held as a DataFrame

    python tools/bam_speed.py [--reads 2000000] [--jobs 4] [--reps 3] [--dir DIR] [--inflate host|device] [--level 1]
                               [--frame host|device] [--segment-bytes N] [--cases se,pe] [--pair host|device]
                               [--pairing name|flag] [--stranded no|forward|reverse]

--level is the deflate level of the written files (the fixture writer's level 1 on random sequence bytes is nearly
literal-only; real files are level 6 and full of matches).  Files found in --dir from an earlier run with the same
--reads and --level are used again.  Every case reports its best repetition (by e2e_ms) and, as *_min / *_max, the
spread of inflate_ms, coverage_ms, pair_device_ms and e2e_ms over the repetitions.  Prints one JSON line.  Needs a GPU.
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
import _flag_cases as fc                             # noqa: E402
import _reads_fixtures as rf                         # noqa: E402
from degnorm_amd import bam                          # noqa: E402
from degnorm_amd import reads as dr                  # noqa: E402


def _best(path, chrom, ov, gene_df, exon_df, out, jobs, reps, inflate, frame='host', segment_bytes=None, verify=False, pair='host',
          pairing='name', stranded='no'):
    best, rows = None, []
    shutil.rmtree(out, ignore_errors=True)            # of an earlier run in the same --dir: files that exist are not written again
    for k in range(reps + 1):                        # the first run loads the library and warms the device up
        proc = bam.NativeBamReadsProcessor(path, path + '.bai', output_dir=os.path.join(out, str(k)), n_jobs=jobs, verbose=False,
                                           inflate=inflate, frame=frame, frame_segment_bytes=segment_bytes, verify=verify, pair=pair,
                                           pairing=pairing, stranded=stranded)
        if k == 0 and path.rsplit(os.sep, 1)[-1].startswith('pe'):
            assert proc.paired, 'the paired file was taken for single-end'
        os.makedirs(proc.save_dir, exist_ok=True)
        proc.timing = {}
        t0 = time.perf_counter()
        proc.chromosome_coverage_read_counts(ov, gene_df, exon_df, chrom)
        e2e = time.perf_counter() - t0
        t = proc.timing
        row = {'inflate_ms': 1e3 * t.get('inflate_s', 0), 'inflate_device_ms': t.get('inflate_device_ms', 0),
               'frame_ms': 1e3 * t.get('frame_s', 0), 'frame_device_ms': t.get('frame_device_ms', 0),
               'frame_fixups': t.get('frame_fixups', 0), 'upload_ms': 1e3 * t.get('upload_s', 0), 'decode_ms': 1e3 * t.get('decode_s', 0),
               'coverage_ms': 1e3 * t.get('coverage_s', 0), 'coverage_device_ms': t.get('coverage_device_ms', 0), 'pair_device_ms': t.get('pair_device_ms', 0),
               'e2e_ms': 1e3 * e2e}
        if k > 0:
            rows.append(row)
            if best is None or row['e2e_ms'] < best['e2e_ms']:
                best = row
    best = {key: round(v, 3 if key.endswith('device_ms') else 1) for key, v in best.items()}
    for key in ('inflate_ms', 'frame_ms', 'frame_device_ms', 'coverage_ms', 'pair_device_ms', 'e2e_ms'):
        best[key + '_min'] = round(min(r[key] for r in rows), 3 if key.endswith('device_ms') else 1)
        best[key + '_max'] = round(max(r[key] for r in rows), 3 if key.endswith('device_ms') else 1)
    if inflate == 'device':                          # the kernel's own spread: what --verify is held against
        best['inflate_device_ms_min'] = round(min(r['inflate_device_ms'] for r in rows), 3)
        best['inflate_device_ms_max'] = round(max(r['inflate_device_ms'] for r in rows), 3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=2_000_000)
    ap.add_argument('--jobs', type=int, default=4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--dir', default=None)
    ap.add_argument('--inflate', choices=['host', 'device'], default='host')
    ap.add_argument('--level', type=int, default=1)
    ap.add_argument('--frame', choices=['host', 'device'], default='host')
    ap.add_argument('--segment-bytes', type=int, default=None, help='segment size of --frame device (default: the library\'s)')
    ap.add_argument('--pair', choices=['host', 'device'], default='host', help='where the mates of the paired case are paired')
    ap.add_argument('--pairing', choices=['name', 'flag'], default='name',
                    help='flag: the paired case is written with equal names, FLAG bits and PNEXT, and paired by FLAG (on the device)')
    ap.add_argument('--cases', default='se,pe', help='se, pe or se,pe')
    ap.add_argument('--stranded', choices=['no', 'forward', 'reverse'], default='no',
                    help='count by strand: the genes alternate strands, the files carry strand bits (mates of a pair agree), and '
                         'coverage_ms / coverage_device_ms are those of the two per-strand calls')
    ap.add_argument('--verify', action='store_true', help='check every BGZF block against the CRC32 of its trailer')
    a = ap.parse_args()
    reads, chrom_len, ov, gene_df, exon_df = rf.scale_case(n_reads=a.reads)
    work = a.dir or tempfile.mkdtemp(prefix='bam_speed_')
    try:
        se = pd.DataFrame({'ref': 0, 'pos': reads.pos.values, 'qname': reads.qname.astype(str).values, 'cigar': reads.cigar.values})
        pe = se.assign(qname=['{0}.{1}'.format(i // 2, 1 + i % 2) for i in range(len(se))], next_ref=0)
        if a.pairing == 'flag':
            n, strand = len(se), np.random.default_rng(1).choice([0x0, 0x10, 0x20], len(se))
            mate = np.arange(n) ^ 1
            mate[mate >= n] = n - 1                  # an odd count: the last read names itself, and is its key's only row
            pe = se.assign(qname=[str(i // 2) for i in range(n)], next_ref=0, flag=0x1 | np.where(np.arange(n) % 2 == 0, 0x40, 0x80) | strand,
                           next_pos=se.pos.values[mate], mapq=60)
        if a.stranded != 'no':
            # a strand per gene, and strand bits in the files: a random 0x10 per fragment, which the last mate of a pair
            # carries inverted, so that both mates say one sense
            gene_df = gene_df.assign(strand=np.where(np.arange(len(gene_df)) % 2 == 0, '+', '-'))
            rev = np.random.default_rng(2).choice([0x0, 0x10], len(se))
            se = se.assign(flag=rev)
            pe = pe.assign(flag=(pe.flag.values & ~0x30 if 'flag' in pe else 0) | (rev[(np.arange(len(se)) // 2) * 2] ^ np.where(np.arange(len(se)) % 2 == 1, 0x10, 0x0)))
        t0 = time.perf_counter()
        cases = [c for c in ('se', 'pe') if c in a.cases.split(',')]
        files = {name: os.path.join(work, '{0}_{1}_l{2}.bam'.format(name + ('_flag' if name == 'pe' and a.pairing == 'flag' else '') +
                                                                     ('_strand' if a.stranded != 'no' else ''), a.reads, a.level))
                 for name in cases}
        for name, df in (('se', se), ('pe', pe)):
            if name in files and not (os.path.isfile(files[name]) and os.path.isfile(files[name] + '.bai')):
                (fc.write_bam if 'next_pos' in df else bf.write_bam)(files[name], [('chrS', chrom_len)], df, level=a.level)
        write_s = time.perf_counter() - t0
        inflated = {name: int(bam.bgzf_blocks(files[name])[2].sum()) for name in files}
        in_mem = None
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            dr.chromosome_coverage_read_counts_df(reads, chrom_len, ov, gene_df, exon_df, False)
            dt = time.perf_counter() - t0
            in_mem = dt if in_mem is None else min(in_mem, dt)
        out = {'tool': 'bam_speed', 'reads': a.reads, 'jobs': a.jobs, 'inflate': a.inflate, 'frame': a.frame, 'pair': a.pair, 'pairing': a.pairing, 'stranded': a.stranded, 'level': a.level,
               'bam_mb': round(os.path.getsize(files[cases[0]]) / 2 ** 20, 1), 'inflated_mb': round(inflated[cases[0]] / 2 ** 20, 1),
               'write_s': round(write_s, 1)}
        if a.verify:
            out['verify'] = True
        if a.pairing == 'flag' and 'pe' in files:
            # what the default (pairing by name) makes of this file: it takes it for single-end, so every pair whose two mates
            # it counts is counted as two reads.  On the host: the in-memory path on the same rows, single-end against paired.
            both = pe.assign(qname_unpaired=pe.qname)
            as_reads = dr.chromosome_coverage_read_counts_df(both, chrom_len, ov, gene_df, exon_df, False)[2]
            as_pairs = dr.chromosome_coverage_read_counts_df(both.sort_values('qname_unpaired', kind='stable'), chrom_len, ov, gene_df, exon_df, True)[2]
            out['default_counts_as_reads'], out['pairs_counted'] = int(sum(as_reads.values())), int(sum(as_pairs.values()))
        for name in cases:
            row = _best(files[name], 'chrS', ov, gene_df, exon_df, os.path.join(work, 'out_{0}_{1}_{2}_{3}'.format(name, a.inflate, a.frame, a.pair)),
                        a.jobs, a.reps, a.inflate, a.frame, a.segment_bytes, a.verify, a.pair, a.pairing if name == 'pe' else 'name', a.stranded)
            if row['inflate_device_ms'] > 0:
                row['inflate_gbps'] = round(inflated[name] / (row['inflate_device_ms'] * 1e-3) / 1e9, 2)
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

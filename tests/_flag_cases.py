"""
Fixtures for the tests of pairing by FLAG and of the read filters (bam.mate_rows, DeviceRows(pairing='flag'),
NativeBamReadsProcessor(pairing=..., exclude_flags=..., require_flags=..., min_mapq=...)).

_bam_fixtures.encode_records writes MAPQ 60 and next_pos = pos; here the rows may carry `mapq` and `next_pos` columns, which
encode() patches into the encoded records (byte 13 and bytes 28 .. 31 of a record), and write_bam() writes a file of such
records.  sam_text() gives the same rows as SAM lines for the tests that go through the converter.  restate() is the numpy
statement of the order and the ids of the FLAG rule, flag_style() turns the synthetic pairs of _reads_fixtures into what an
aligner writes (equal names, FLAG bits, PNEXT) next to their twin under the name rule (names g<k>.1 / g<k>.2).
"""
import struct

import numpy as np
import pandas as pd

import _bam_fixtures as bf

PAIRED, PROPER, UNMAPPED, MATE_UNMAPPED, REVERSE, MATE_REVERSE, FIRST, LAST = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
SECONDARY, QCFAIL, DUP, SUPPLEMENTARY = 0x100, 0x200, 0x400, 0x800
_encode_records = bf.encode_records                    # write_bam() below puts encode() in its place for a call


def padded(names):
    """The names (bytes) as a fixed-width S array: NUL padded, compared as unsigned bytes."""
    names = [bytes(k) for k in names]
    width = max([len(k) for k in names] + [1])
    return np.array(names, dtype='S{0}'.format(width)) if names else np.zeros(0, dtype='S1')


def restate(names, pos, next_pos, flag):
    """
    (order, pair_id, number of ids) of the FLAG rule by numpy: a stable lexsort by padded name, then (uint32) (pos_first + 1),
    then (uint32) (pos_last + 1), and the count of key changes before each position.  A row with 0x40 is a first mate.
    """
    a = padded(names)
    pos, next_pos, flag = np.asarray(pos, np.int64), np.asarray(next_pos, np.int64), np.asarray(flag, np.int64)
    if len(a) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    first = (flag & FIRST) != 0
    kf = (np.where(first, pos, next_pos) + 1) & 0xffffffff
    kl = (np.where(first, next_pos, pos) + 1) & 0xffffffff
    order = np.lexsort((kl, kf, a))                            # stable; the last key is the primary one
    sa, sf, sl = a[order], kf[order], kl[order]
    change = (sa[1:] != sa[:-1]) | (sf[1:] != sf[:-1]) | (sl[1:] != sl[:-1])
    pair_id = np.r_[0, np.cumsum(change)]
    return order, pair_id, int(pair_id[-1]) + 1


def rows(records, ref=0):
    """A DataFrame for encode() / write_bam() from (qname, pos, cigar, flag, next_pos[, next_ref[, mapq]]) tuples."""
    full = [tuple(r) + (ref, 60)[len(r) - 5:] for r in records]
    return pd.DataFrame(full, columns=['qname', 'pos', 'cigar', 'flag', 'next_pos', 'next_ref', 'mapq']).assign(ref=ref)


def encode(reads, seed=0):
    """_bam_fixtures.encode_records with the rows' `mapq` and `next_pos` columns (where there are any) patched in."""
    data, offs = _encode_records(reads, seed)
    data = bytearray(data)
    if 'mapq' in reads:
        for o, q in zip(offs.tolist(), reads['mapq'].tolist()):
            data[o + 13] = int(q)
    if 'next_pos' in reads:
        for o, p in zip(offs.tolist(), reads['next_pos'].tolist()):
            data[o + 28:o + 32] = struct.pack('<i', int(p))
    return bytes(data), offs


def write_bam(path, refs, reads, **kw):
    """_bam_fixtures.write_bam on records encoded by encode(): the same file layout and index."""
    bf.encode_records = encode
    try:
        return bf.write_bam(path, refs, reads, **kw)
    finally:
        bf.encode_records = _encode_records


def aux_offset(data, o):
    """Where the aux fields of the record at offset o begin."""
    l_name, n_cig = data[o + 12], struct.unpack_from('<H', data, o + 16)[0]
    l_seq = struct.unpack_from('<i', data, o + 20)[0]
    return o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def sam_text(reads, refs):
    """The rows, in the order given, as SAM alignment lines (str): FLAG, MAPQ, RNEXT and PNEXT from their columns."""
    lines = []
    name = lambda r: '*' if r < 0 else refs[r][0]                                            # noqa: E731
    for q, f, ref, pos, mq, cig, nref, npos in zip(reads['qname'].tolist(), reads['flag'].tolist(), reads['ref'].tolist(), reads['pos'].tolist(),
                                                   reads['mapq'].tolist(), reads['cigar'].tolist(), reads['next_ref'].tolist(),
                                                   reads['next_pos'].tolist()):
        cig = cig if isinstance(cig, str) and cig else '*'
        qlen = bf._binary_cigar(cig)[2] if cig != '*' else 0
        rnext = '*' if nref < 0 else '=' if nref == ref else name(nref)
        lines.append('\t'.join([q, str(f), name(ref), str(pos + 1), str(mq), cig, rnext, str(npos + 1), '0',
                                'A' * qlen or '*', 'I' * qlen or '*']))
    return ''.join(ln + '\n' for ln in lines)


def sam_header(refs):
    return '@HD\tVN:1.6\n' + ''.join('@SQ\tSN:{0}\tLN:{1}\n'.format(nm, ln) for nm, ln in refs) + '@PG\tID:aligner\n'


def flag_style(src, ref=0, other_ref=1, seed=0, elsewhere=0.05):
    """
    The pairs of _reads_fixtures.synth_pairs (names p<k>.1 / p<k>.2, a few orphans) as an aligner writes them, and their
    twin: (flagged, twin), two DataFrames of the same records in the same order that differ in `qname` only -- g<k> for both
    mates against g<k>.1 / g<k>.2.  A first mate gets 0x41, a last one 0x81, both a random share of the strand bits and 0x2,
    and next_pos is the mate's pos.  An orphan gets 0x8 and next_ref = ref (the name rule keeps it and finds its name once;
    the FLAG rule does not store it).  A share `elsewhere` of the pairs has its second mate on other_ref: the name rule finds
    the first mate's name once on `ref`, the FLAG rule does not store it.
    """
    rng = np.random.default_rng(seed)
    out = []
    for k, (_, g) in enumerate(src.groupby('qname_unpaired', sort=False)):
        mates = list(zip(g.qname.tolist(), g.pos.tolist(), g.cigar.tolist()))
        away = len(mates) == 2 and rng.random() < elsewhere
        for j, (q, pos, cig) in enumerate(mates):
            f = PAIRED | (FIRST if q.endswith('.1') else LAST) | int(rng.choice([0, REVERSE, MATE_REVERSE, PROPER, PROPER | REVERSE]))
            if len(mates) == 1:
                out.append(('g{0}'.format(k), q[-2:], ref, pos, cig, f | MATE_UNMAPPED, ref, pos))
                continue
            here, there = (other_ref if away and j == 1 else ref), (other_ref if away and j == 0 else ref)
            out.append(('g{0}'.format(k), q[-2:], here, pos, cig, f, there, mates[1 - j][1]))
    df = pd.DataFrame(out, columns=['qname', 'suffix', 'ref', 'pos', 'cigar', 'flag', 'next_ref', 'next_pos']).assign(mapq=60)
    twin = df.assign(qname=df.qname + df.suffix)
    return df.drop(columns='suffix'), twin.drop(columns='suffix')


def random_mates(n, n_names, seed, max_len=12, span=6):
    """
    n flag-style rows in file order (pos ascending) for the store-level tests: names from a pool of n_names (0 .. max_len
    bytes, so that some are prefixes of others), positions and mate positions from a range narrow enough that keys repeat, and
    0x41 or 0x81 with strand bits -- DataFrame(ref, pos, qname, cigar, flag, next_ref, next_pos, mapq).
    """
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b'abc', dtype=np.uint8)
    pool = sorted(set(alpha[rng.integers(0, 3, int(rng.integers(1, max_len + 1)))].tobytes().decode() for _ in range(4 * n_names)))[:n_names]
    names = [pool[i] for i in rng.integers(0, len(pool), n)]
    pos = np.sort(rng.integers(0, span, n))
    flag = PAIRED | np.where(rng.random(n) < 0.5, FIRST, LAST) | rng.choice([0, REVERSE, MATE_REVERSE], n)
    return pd.DataFrame({'ref': 0, 'pos': pos, 'qname': names, 'cigar': '20M', 'flag': flag, 'next_ref': 0,
                         'next_pos': rng.integers(0, span, n), 'mapq': rng.integers(0, 256, n)})

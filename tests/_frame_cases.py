"""
Inputs for the tests of segmented record framing (csrc/dn_frame.hip), shared by test_frame_host.py (the host build, no GPU)
and test_gpu_frame.py (the kernels).  Every case is (name, bytes, tid, last_pos); the yardstick is the serial walk,
bam.frame_records(buf, tid, last_pos): offsets, bytes consumed, last pos and error texts must be equal, at every segment
size of SEGMENTS (0: the library's default).

    valid_cases()     3 000 mixed records whole, cut at 40 seeded points (inside block_size, inside the fixed 32 bytes,
                      mid-payload) and the edges; a record longer than three 4 096-byte segments; records with empty
                      read names, which the guess rule refuses although they are true records; the decoys
    decoys(variant)   400 records whose last aux field is a B:C array holding a complete valid record of the same refID:
                      'last' -- the decoy ends where its host record ends, so a walk from it rejoins the true chain;
                      'mid' -- four more aux bytes follow, so a walk from it runs into garbage.  A B:C pad of seeded
                      length 0 .. 89 before the decoy puts the segment boundaries at all phases
    error_cases(S)    block_size 0, -5 and 31 in the middle and at the tail, pos stepping back (mid-segment, at the first
                      record of a segment of S bytes, against last_pos), a wrong refID, and two errors in one buffer
"""
import struct

import numpy as np
import pandas as pd

import _bam_fixtures as bf

SEGMENTS = (64, 256, 4096, 0)
INT32_MIN = -2 ** 31
_CIGARS = ['20M', '12M3I9M', '5S15M200N10M', '8M1D8M1I8M', '30M', '4M2000N4M2000N4M2000N4M', '10M5H', '3=2X10M', '25M']


def mixed_frame(n, seed, ref=0):
    """n rows for _bam_fixtures.encode_records: sorted pos, cigars and names of differing length, NH of every integer type."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, 5_000_000, n))
    return pd.DataFrame({'ref': ref, 'pos': pos, 'qname': ['q' * int(rng.integers(1, 9)) + str(i) for i in range(n)],
                         'cigar': rng.choice(_CIGARS, n), 'nh': rng.choice([1, 2, None], n).tolist(),
                         'nh_type': rng.choice(['C', 'S', 'i', 'c', 's', 'I'], n).tolist(), 'next_ref': rng.choice([-1, ref], n)})


def mixed(n=3000, seed=11):
    return bf.encode_records(mixed_frame(n, seed), seed)


def cuts(buf, offs, n=40, seed=5):
    """n seeded cut points of buf: inside a block_size, inside the fixed 32 bytes after it, and mid-payload, in turn."""
    rng = np.random.default_rng(seed)
    ends = np.append(offs[1:], len(buf))
    out = []
    for j, k in enumerate(rng.choice(len(offs), n, replace=False).tolist()):
        lo, hi = [(1, 4), (4, 36), (36, int(ends[k] - offs[k]))][j % 3]
        out.append(int(offs[k]) + int(rng.integers(lo, hi)))
    return sorted(out)


def long_record():
    """Ordinary records around one of l_seq 20 000 (30 KB: segments of 4 096 bytes with no record start in them)."""
    df = mixed_frame(61, 3)
    df.loc[30, 'cigar'] = '20000M'
    return bf.encode_records(df, 3)


def decoys(variant, n=400, seed=17, tid=0):
    rng = np.random.default_rng(seed)
    df = mixed_frame(n, seed, ref=tid)
    data, offs = bf.encode_records(df, seed)
    ends = np.append(offs[1:], len(data)).tolist()
    inner = mixed_frame(n, seed + 1, ref=tid)
    out, starts, o = [], [], 0
    for k, (a, b) in enumerate(zip(offs.tolist(), ends)):
        decoy = bf.encode_records(inner.iloc[k:k + 1], seed)[0]
        pad = int(rng.integers(0, 90))
        extra = b'XPBC' + struct.pack('<i', pad) + b'\xff' * pad + b'XDBC' + struct.pack('<i', len(decoy)) + decoy
        if variant == 'mid':
            extra += b'XCC\x07'
        else:
            assert variant == 'last'
        body = data[a + 4:b] + extra
        out.append(struct.pack('<i', len(body)) + body)
        starts.append(o)
        o += 4 + len(body)
    return b''.join(out), np.array(starts, np.int64)


def valid_cases():
    buf, offs = mixed()
    cases = [('whole', buf, 0, INT32_MIN), ('whole_any_ref', buf, -1, INT32_MIN)]
    cases += [('cut{0}'.format(c), buf[:c], 0, INT32_MIN) for c in cuts(buf, offs)]
    one = int(offs[1])
    cases += [('empty', b'', 0, INT32_MIN), ('b1', buf[:1], 0, INT32_MIN), ('b2', buf[:2], 0, INT32_MIN), ('b3', buf[:3], 0, INT32_MIN),
              ('one', buf[:one], 0, INT32_MIN), ('one_plus3', buf[:one + 3], 0, INT32_MIN)]
    cases.append(('long', long_record()[0], 0, INT32_MIN))
    # true records the guess rule refuses (empty read names, l_read_name 1): their segments must come right by fix-up
    cases.append(('empty_names', bf.encode_records(mixed_frame(300, 29).assign(qname=''), 29)[0], 0, INT32_MIN))
    for v in ('last', 'mid'):
        d = decoys(v)[0]
        cases += [('decoy_' + v, d, 0, INT32_MIN), ('decoy_any_ref_' + v, d, -1, INT32_MIN)]
    return cases


def _patched(buf, at, fmt, value):
    b = bytearray(buf)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def error_cases(segment_bytes):
    """Buffers the serial walk refuses (and, with tid -1, frames without the order checks); see the module docstring."""
    S = segment_bytes or 16384
    buf, offs = bf.encode_records(mixed_frame(600, 23), 23)
    offs = offs.tolist()
    pos = [struct.unpack_from('<i', buf, o + 8)[0] for o in offs]
    mid = 300
    first = next(k for k in range(1, len(offs)) if offs[k] // S != offs[k - 1] // S)      # the first record of a segment
    # a record that is not the first of its segment (segments shorter than a record hold no such record: any one then)
    inner = next((k for k in range(2, len(offs)) if offs[k] // S == offs[k - 1] // S), mid + 7)
    cases = []
    for bs in (0, -5, 31):
        bad = _patched(buf, offs[mid], '<i', bs)
        cases.append(('bs{0}_mid'.format(bs), bad, 0, INT32_MIN))
        for visible in (4, 20, 35):
            cases.append(('bs{0}_tail{1}'.format(bs, visible), bad[:offs[mid] + visible], 0, INT32_MIN))
    back_inner = _patched(buf, offs[inner] + 8, '<i', pos[inner - 1] - 1)
    back_first = _patched(buf, offs[first] + 8, '<i', pos[first - 1] - 1)
    wrong_ref = _patched(buf, offs[mid] + 4, '<i', 1)
    cases += [('pos_back_mid_segment', back_inner, 0, INT32_MIN), ('pos_back_first_of_segment', back_first, 0, INT32_MIN),
              ('pos_back_against_last_pos', buf, 0, pos[0] + 1), ('wrong_ref', wrong_ref, 0, INT32_MIN),
              ('sort_then_malformed', _patched(_patched(buf, offs[100] + 8, '<i', pos[99] - 1), offs[400], '<i', 7), 0, INT32_MIN),
              ('malformed_then_sort', _patched(_patched(buf, offs[400] + 8, '<i', pos[399] - 1), offs[100], '<i', 7), 0, INT32_MIN)]
    cases += [(name + '_any_ref', b, -1, lp) for name, b, _, lp in cases[-6:]]
    return cases


def outcome(frame, buf, tid, last_pos, **kw):
    """What a framing call gives: ('ok', offsets, consumed, last pos) or ('error', the ValueError's text)."""
    try:
        off, used, last = frame(buf, tid, last_pos, **kw)
    except ValueError as e:
        return ('error', str(e))
    return ('ok', off.tolist(), used, last)

"""
Cases and an independent builder for the tests of the .csi index (degnorm_amd.bam.build_index(fmt='csi')); numpy, pandas,
struct and zlib only, the library is never called here.  The shared pieces -- records, block layouts, virtual offsets --
are those of tests/_bai_cases.py.

    spec_index(refs, records, blocks, min_shift, depth)   the inflated bytes of the canonical .csi of include/degnorm_amd.h,
                                                          record by record, in plain Python
    auto_depth(refs, min_shift)                           the depth build_index(depth=None) must take
    regions(name, refs, reads, n, seed)                   seeded (tid, beg, end) at the scale of case `name`

Cases (CASES: name -> (min_shift, depth or None, builder)):
    levels   (4, 3): a reference of 8 192 bases, the cap of that index, and a short one; reads of 1 .. 8 191 bases in the bins of
             every level, reads that straddle each level's boundaries by one base, one that ends at the cap
    wide     (4, 6): references of 2^21 + 5 000 bases, that is more than 65 536 granules of 16 bases: reads around granule
             65 535 / 65 536, one spliced read from granule 10 to granule 131 100, reads at the end; a second reference of
             the same length without that read, so that claims beyond granule 65 535 occur one by one
    beyond   depth=None, which comes out as 6 at min_shift 14: a reference of 2^29 + 2^16 bases before one of 100 kb: reads
             that end at 2^29, start at 2^29 - 1 and at 2^29, a 40 kb splice across it, reads up to the last base
"""
import struct

import numpy as np

import _bai_cases as bc
import _bam_fixtures as bf

COUNTS = (1, 255, 256, 257)             # streams around the 256 lanes of the kernels' workgroups


def level_table(min_shift, depth):
    """[(level, first bin t_l, shift s_l of the bins' span)], the root first."""
    return [(l, ((1 << 3 * l) - 1) // 7, min_shift + 3 * (depth - l)) for l in range(depth + 1)]


def reg2bin(beg, end, min_shift, depth):
    l, s, t = depth, min_shift, ((1 << 3 * depth) - 1) // 7
    end -= 1
    while l > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        l -= 1
        s += 3
        t -= 1 << 3 * l
    return 0


def bin_level(b, min_shift, depth):
    """(level, start of the interval) of bin b."""
    l, t, s = [row for row in level_table(min_shift, depth) if row[1] <= b][-1]
    return l, (b - t) << s


def pseudo_bin(depth):
    return ((1 << 3 * (depth + 1)) - 1) // 7 + 1


def auto_depth(refs, min_shift=14):
    longest, depth = max(length for _, length in refs), 0
    while 1 << (min_shift + 3 * depth) < longest + 256:
        depth += 1
    return depth


def spec_index(refs, records, blocks, min_shift, depth):
    n_ref = len(refs)
    cap = 1 << (min_shift + 3 * depth)
    bins = [dict() for _ in range(n_ref)]            # bin -> chunks in file order
    rows = [[] for _ in range(n_ref)]                # (end, vbeg) of the reference's records in file order
    meta = [None] * n_ref
    n_no_coor, prev = 0, None
    for ref, beg, end, flag, s, e in bc.record_table(records):
        vb, ve = bc.voffset(blocks, s), bc.voffset(blocks, e)
        if ref < 0:
            n_no_coor += 1
            prev = None
            continue
        assert beg <= cap and end <= cap
        b = reg2bin(beg, end, min_shift, depth)
        if prev == (ref, b):
            bins[ref][b][-1][1] = ve
        else:
            bins[ref].setdefault(b, []).append([vb, ve])
        prev = (ref, b)
        if meta[ref] is None:
            meta[ref] = [vb, ve, 0, 0]
        meta[ref][1] = ve
        meta[ref][3 if flag & 4 else 2] += 1
        rows[ref].append((end, vb))
    out = bytearray(b'CSI\x01' + struct.pack('<iiii', min_shift, depth, 0, n_ref))
    for r in range(n_ref):
        if meta[r] is None:
            out += struct.pack('<i', 0)
            continue
        ends = np.array([x[0] for x in rows[r]], dtype=np.int64)
        out += struct.pack('<i', len(bins[r]) + 1)
        for b in sorted(bins[r]):
            merged = []
            for vb, ve in bins[r][b]:
                if merged and merged[-1][1] >> 16 >= vb >> 16:
                    merged[-1][1] = ve
                else:
                    merged.append([vb, ve])
            # the first record of the reference, in file order, whose end lies beyond the start of the bin's interval
            first = int(np.argmax(ends > bin_level(b, min_shift, depth)[1]))
            assert ends[first] > bin_level(b, min_shift, depth)[1]
            out += struct.pack('<IQi', b, rows[r][first][1], len(merged))
            for vb, ve in merged:
                out += struct.pack('<QQ', vb, ve)
        out += struct.pack('<IQi', pseudo_bin(depth), 0, 2) + struct.pack('<QQQQ', *meta[r])
    out += struct.pack('<Q', n_no_coor)
    return bytes(out)


def spliced(length):
    """A CIGAR that spans `length` reference bases with at most 50 read bases."""
    return '{0}M'.format(length) if length <= 50 else '20M{0}N20M'.format(length - 40)


def _reads(ref, pos, length):
    return bc._frame(ref, np.asarray(pos, dtype=np.int64), [spliced(int(x)) for x in np.broadcast_to(length, np.shape(pos))])


def case_levels():
    rng = np.random.default_rng(21)
    cap = 1 << 13
    refs = [('chrC', cap), ('chrT', 500)]
    n = 2400
    length = rng.choice([1, 5, 16, 17, 100, 128, 129, 1000, 1024, 1025, 3000, 8191], n)
    pos = np.minimum(rng.integers(0, cap, n), cap - length)
    parts = [_reads(0, pos, length)]
    for s in (4, 7, 10):                                                  # one base on either side of each level's boundaries
        edge = np.arange(1, cap >> s, max(1, (cap >> s) // 16)) << s
        parts += [_reads(0, edge - 1, 2), _reads(0, edge - 1, 1), _reads(0, edge, 1), _reads(0, edge - (1 << s), 1 << s)]
    parts += [_reads(0, [1, cap - 50, cap - 1, 0], [8191, 50, 1, 8191])]  # ends at the cap
    parts.append(bc._frame(0, rng.integers(0, cap - 1, 30), None, 4))
    parts.append(_reads(1, np.sort(rng.integers(0, 450, 200)), 40))
    parts.append(bc._frame(-1, np.full(20, -1), None, 4))
    return refs, bc._finish(parts)


def case_wide():
    rng = np.random.default_rng(22)
    L, g = (1 << 21) + 5000, 16
    refs = [('chrW', L), ('chrX', L)]
    parts = []
    for ref in (0, 1):
        parts.append(_reads(ref, rng.integers(0, L - 3000, 1100), rng.choice([1, 16, 50, 300, 2500], 1100)))
        parts.append(_reads(ref, [0, 0, 65536 * g - 50, 65536 * g - 1, 65536 * g, 65536 * g + 3], [50, 1, 50, 2, 50, 16]))
        parts.append(_reads(ref, [L - 50, L - 1, L - 3000], [50, 1, 3000]))
    parts.append(_reads(0, [10 * g], [131100 * g + 3 - 10 * g + 1]))       # from granule 10 to granule 131 100
    return refs, bc._finish(parts)


def case_beyond():
    rng = np.random.default_rng(23)
    H = 1 << 29
    L = H + (1 << 16)
    refs = [('chrH', L), ('chrS', 100000)]
    parts = [_reads(0, rng.integers(0, 1 << 20, 300), 50)]
    parts.append(_reads(0, rng.integers(H - (1 << 21), L - 41000, 1700), rng.choice([50, 50, 400, 40050], 1700)))
    parts.append(_reads(0, [H - 50, H - 1, H - 1, H, H, H - 20000, L - 50, L - 1], [50, 1, 2, 50, 1, 40050, 50, 1]))
    parts.append(bc._frame(0, rng.integers(H, L - 1, 20), None, 4))
    parts.append(_reads(1, np.sort(rng.integers(0, 99000, 300)), 50))
    return refs, bc._finish(parts)


CASES = {'levels': (4, 3, case_levels), 'wide': (4, 6, case_wide), 'beyond': (14, None, case_beyond)}
# the cases of tests/_bai_cases.py, at the .bai's own scheme and with the depth left open
SHARED = [(name, 14, depth) for name in sorted(bc.CASES) for depth in (5, None)]


def case_count(n):
    """n reads on one reference of 2^29 + 2^16 bases, the last of them beyond 2^29."""
    H = 1 << 29
    pos = np.arange(n) * 5000
    pos[-1] = H + 100
    return [('chrH', H + (1 << 16))], bc._finish([_reads(0, pos, 50)])


def long_cigar(length):
    """A CIGAR of `length` reference bases and one read base: an N op holds at most 2^28 - 1."""
    ops, rest = ['1M'], length - 1
    while rest > 0:
        ops.append('{0}N'.format(min(rest, (1 << 28) - 1)))
        rest -= min(rest, (1 << 28) - 1)
    return ''.join(ops)


def range_file(path, min_shift, depth, extra, n=700):
    """
    n reads and then one that ends `extra` bases beyond the cap of (min_shift, depth), which is record n: (its position, the
    text build_index must give for extra > 0).
    """
    cap = 1 << (min_shift + 3 * depth)
    good = bc._frame(0, np.sort(np.random.default_rng(3).integers(0, min(cap, 1 << 20) - 60, n)), '50M')
    pos = min(cap - 50, (1 << 31) - 100)
    frame = bc._finish([good, bc._frame(0, [pos], [long_cigar(cap - pos + extra)])])
    assert bc.span(0, pos, 0, frame.cigar.iloc[-1]) == (pos, cap + extra) and frame.pos.iloc[-1] == pos
    data, offs = bf.encode_records(frame)
    hdr = bf.header_bytes([('chrA', 1000)])
    bc.write_layout(path, hdr, data, bc.layout_cuts('straddle', len(hdr), offs, len(data)), 1)
    return pos, ('{0}: record {1} (refID 0, position {2}) reaches beyond position 2^{3}: a .csi index of min_shift {4} and depth {5} '
                 'cannot hold it'.format(path, n, pos, min_shift + 3 * depth, min_shift, depth))


RANGE_PARAMS = [(14, 5), (4, 3), (14, 6)]


def build_case(name, layout, path, level=1):
    """Write case `name` (of CASES, of _bai_cases.CASES, or ('count', n)) in `layout`: (refs, records, blocks, sorted reads)."""
    if isinstance(name, tuple):
        refs, reads = case_count(name[1])
    else:
        refs, reads = CASES[name][2]() if name in CASES else bc.CASES[name]()
    data, offs = bf.encode_records(reads)
    hdr = bf.header_bytes(refs)
    blocks = bc.write_layout(path, hdr, data, bc.layout_cuts(layout, len(hdr), offs, len(data)), level)
    return refs, (reads, offs + len(hdr), len(hdr) + len(data)), blocks, reads


def regions(name, refs, reads, n, seed, min_shift, depth):
    """
    n seeded (tid, beg, end) on references that have reads: two thirds anywhere, of the sizes of the index's levels; a third
    within two bases of a granule or level boundary (the .bai's cap 2^29 is one of `beyond`).
    """
    rng = np.random.default_rng(seed)
    tids = sorted(set(int(r) for r in reads['ref'] if r >= 0))
    sizes = [1, 3] + [1 << s for _, _, s in level_table(min_shift, depth)] + [(1 << min_shift) + 1]
    out = []
    for k in range(n):
        tid = int(rng.choice(tids))
        length = refs[tid][1]
        size = int(rng.choice(sizes))
        if k % 3 == 2:
            s = int(rng.choice([row[2] for row in level_table(min_shift, depth)[1:]]))
            edge = int(rng.integers(1, max(2, length >> s) + 1)) << s
            beg = max(0, min(edge, length) + int(rng.integers(-2, 3)))
            if name == 'beyond' and tid == 0 and k % 2:
                beg = (1 << 29) + int(rng.integers(-2, 3)) - (size if k % 4 == 1 else 0)
        elif name == 'beyond' and tid == 0 and k % 3 == 1:       # where that case has its reads: the first megabase and the end
            beg = int(rng.integers(0, 1 << 20)) if k % 2 else int(rng.integers((1 << 29) - (1 << 21), length))
        else:
            beg = int(rng.integers(0, length))
        out.append((tid, beg, max(beg + 1, min(beg + size, length))))
    return out

"""
Key sets for the tests of mate pairing (bam.pair_rows, DeviceRows.pair): the shapes a qname_unpaired key can take around the
8-byte chunks of the radix passes, the numpy oracle, rows that carry given keys through a BAM file, and the count of the
pairs whose result can depend on the order of their two mates.
"""
import numpy as np
import pandas as pd

WIDTHS = (1, 7, 8, 9, 16, 17, 40)                  # around the chunk boundaries
_ALPHA = np.frombuffer(b'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._-:', dtype=np.uint8)


def as_array(keys):
    """The keys as a fixed-width S array (numpy pads with NUL, compares as unsigned bytes)."""
    keys = list(keys)
    width = max([len(k) for k in keys] + [1])
    return np.array(keys, dtype='S{0}'.format(width)) if keys else np.zeros(0, dtype='S1')


def oracle(keys):
    """(order, pair_id, number of ids) by numpy: the stable argsort and the count of key changes before each position."""
    a = as_array(keys) if not isinstance(keys, np.ndarray) else keys
    order = np.argsort(a, kind='stable')
    sk = a[order]
    pair_id = np.r_[0, np.cumsum(sk[1:] != sk[:-1])] if len(a) else np.zeros(0, dtype=np.int64)
    return order, pair_id, int(pair_id[-1]) + 1 if len(a) else 0


def width_keys(width, n=60, seed=0):
    """n keys of exactly `width` bytes that share all but their last two bytes, so that most occur more than once."""
    rng = np.random.default_rng(seed + width)
    head = _ALPHA[rng.integers(0, len(_ALPHA) - 5, max(width - 2, 0))].tobytes()
    tails = [_ALPHA[rng.integers(0, 3, min(width, 2))].tobytes() for _ in range(n)]
    return [head + t for t in tails]


def random_keys(n, n_distinct, seed=5, high=False, max_len=40):
    """n keys drawn from n_distinct values of 0 .. max_len bytes: printable ones, or (high) any byte but NUL."""
    rng = np.random.default_rng(seed)
    pool = set()
    while len(pool) < n_distinct:
        ln = int(rng.integers(0, max_len + 1))
        pool.add(rng.integers(1, 256, ln).astype(np.uint8).tobytes() if high else _ALPHA[rng.integers(0, len(_ALPHA), ln)].tobytes())
    pool = sorted(pool)
    return [pool[i] for i in rng.integers(0, n_distinct, n)]


def key_sets(high=True):
    """[(name, keys)]: every shape of the issue but the large random set.  high=False leaves out the sets with bytes >= 0x80."""
    rng = np.random.default_rng(1)
    sets = [('n0', []), ('n1', [b'b']), ('n2', [b'b', b'a']), ('n3', [b'b', b'a', b'b'])]
    sets += [('width{0}'.format(w), width_keys(w)) for w in WIDTHS]
    sets.append(('widths_mixed', [k for w in WIDTHS for k in width_keys(w, 12)][::-1]))
    sets.append(('all_equal', [b'same.key'] * 9))
    sets.append(('all_distinct', ['r{0}'.format(i).encode() for i in rng.permutation(300)]))
    for times in (1, 2, 5):
        keys = [b'k3', b'k1', b'k2', b'k1'] * 3
        for at in range(times):
            keys.insert(2 * at + 1, b'')
        sets.append(('empty_x{0}'.format(times), keys))
    sets.append(('prefix', [b'r10', b'r1.a', b'r1', b'r1.a', b'r10', b'r1', b'r', b'r1.a.b']))
    sets.append(('ninth_byte', [b'abcdefgh' + c for c in (b'z', b'a', b'', b'm', b'a', b'zz', b'z')]))
    sets.append(('first_byte', [c + b'-tail-of-11' for c in (b'q', b'b', b'z', b'b', b'a', b'q')]))
    sets.append(('triple', [b't3', b'p1', b't3', b'o1', b'p1', b't3', b'p2', b'p2']))
    if high:
        sets.append(('high_bytes', [b'\x80a', b'\x7fz', b'\xff', b'\x80', b'a\xfe', b'a\x7f', b'\xff\x01', b'\x80a', b'abcdefgh\xc3\xa9', b'abcdefgh\x7f']))
        sets.append(('high_random', random_keys(400, 150, seed=9, high=True, max_len=20)))
    return sets


def rows_for(keys, ref=0, next_ref=0):
    """
    Rows for _bam_fixtures.write_bam / encode_records whose qname_unpaired are the (ASCII) keys, in this order in the file:
    the name is the key, a '.' and the mate number -- for the empty key a name without a '.' -- and pos rises with the row.
    """
    seen, names = {}, []
    for i, k in enumerate(keys):
        seen[k] = seen.get(k, 0) + 1
        names.append((k + b'.' + str(seen[k]).encode()).decode('ascii') if k else 'x{0}'.format(i))
    return pd.DataFrame({'ref': ref, 'pos': 10 + 3 * np.arange(len(keys), dtype=np.int64), 'qname': names, 'cigar': '20M', 'next_ref': next_ref})


def reference_span(pos, cigar):
    """[pos, end) on the reference of a read: M, D, N, = and X advance it."""
    num, end = '', int(pos)
    for ch in cigar or '':
        if ch.isdigit():
            num += ch
        else:
            end += int(num) if ch in 'MDN=X' else 0
            num = ''
    return int(pos), end


def order_sensitive_pairs(qnames, pos, cigars):
    """
    For reads in file order: (pairs, pairs whose mates overlap on the reference, of those the pairs that kind='stable' and
    kind='quicksort' put in different mate order).  A pair is a qname_unpaired (the name up to its last '.') that occurs
    exactly twice, in a file that the reader takes for paired-end: one whose names end, after their last '.', in 1 or 2 and in
    nothing else (BamReadsProcessor.determine_if_paired); any other file has no pairs.
    """
    if set(q.split('.')[-1] for q in qnames) != {'1', '2'}:
        return 0, 0, 0
    keys = as_array([q.rsplit('.', 1)[0].encode() if '.' in q else b'' for q in qnames])
    if len(keys) == 0:
        return 0, 0, 0
    stable, quick = np.argsort(keys, kind='stable'), np.argsort(keys, kind='quicksort')
    sk = keys[stable]
    first = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    size = np.diff(np.r_[first, len(sk)])
    at = first[size == 2]
    assert np.array_equal(keys[quick], sk)
    n_overlap = n_differ = 0
    for k in at.tolist():
        a, b = int(stable[k]), int(stable[k + 1])
        (a0, a1), (b0, b1) = reference_span(pos[a], cigars[a]), reference_span(pos[b], cigars[b])
        if a0 < b1 and b0 < a1:
            n_overlap += 1
            n_differ += int(quick[k]) != a
    return len(at), n_overlap, n_differ

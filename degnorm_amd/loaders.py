"""
Annotation loaders on the device: GTF (GeneAnnotationLoader) and GFF3 (Gff3AnnotationLoader); `annotation_loader` picks one
by the file's extension.

GTF annotation loader on the device (reference: `degnorm/loaders.py:73-168`, GeneAnnotationLoader).

The reference reads the nine columns with pandas, lower-cases the feature column and runs a regex per exon row.  Here the
file's bytes go to the GPU window by window (about window_bytes each, cut at line ends) and `dn_gtf_scan`
(csrc/dn_gtf.hip) returns the exon lines in file order: start, end and the byte spans of the chromosome and gene names
with a hash of each.  The host turns every distinct name into one Python string (names are grouped by hash and length and
then compared byte for byte, so two names that share a hash stay apart) and drops duplicate rows on integer codes.

The gene name of a line follows the reference's `_attribute_to_gene` (loaders.py:102-112): the attribute field is split
at `;`, every piece stripped; the first piece that begins with `gene_name` gives the name, and when there is none or its
value is empty the first piece that begins with `gene_id` does; the value is the rest of the piece without blanks and `"`
at either end.  Narrowings: a blank is the ASCII space; the tag is cut off once, at the front of the piece (the reference
removes every occurrence of the tag's text from the piece); start and end are 1 to 18 decimal digits and nothing else.

Two deliberate differences from the reference: lines that start with `#` and empty lines are skipped (the reference
raises on them, so it refuses every Ensembl or GENCODE download), and `chr` is always the file's text (pandas' type
inference turns a column of `01` into 1).  There is no CPU fallback: without a device `get_data` raises DegnormAmdError.

GFF3 (`dn_gff3_*`, csrc/dn_gff3.hip; include/degnorm_amd.h, "GFF3 annotation scan", defines the rule): an exon line may name
only its Parent, so the gene of an exon is a join over the whole file.  The file's text stays on the device for one load;
every window gives its exon rows -- with the gene's name, or with the Parent still to resolve -- and leaves its node rows
(the lines with an ID) on the device; `dn_gff3_resolve` then walks every pending exon up to its gene.  Spans are offsets in
the file, so names are interned over a memory map of it.  Values are the file's bytes: no percent-decoding.  The same table
comes out as for the GTF twin of the annotation, and like GTF the file loader has no CPU fallback (`gff3_scan` on a buffer has
a host build, which the tests hold to a plain restatement of the rule).
"""
import ctypes
import os
import time

import numpy as np

from . import _lib, gz

WINDOW_BYTES = 256 << 20            # as NativeBamReadsProcessor (bam.py)
_COMPARE_BYTES = 32 << 20           # bytes held at a time when the names of a hash group are compared
_KINDS = {1: 'must have the 9 mandatory .gtf columns.\nRead more at https://useast.ensembl.org/info/website/upload/gff.html',
          2: 'is an exon record without a usable gene_name or gene_id identifier tag.',
          3: 'is an exon record whose start or end is not an integer.',
          4: 'is an exon record whose strand (column 7) is not one of + - . ?'}
_GFF3_KINDS = {1: 'must have the 9 mandatory .gff3 columns.\nRead more at https://github.com/The-Sequence-Ontology/Specifications/blob/master/gff3.md',
               2: 'is an exon record without a usable gene_name, gene, Parent or gene_id attribute.',
               3: 'is an exon record whose start or end is not an integer.',
               4: 'is an exon record whose chain of Parent attributes names an ID that no record has.',
               5: 'is an exon record whose chain of Parent attributes does not reach a gene within 8 records.',
               6: 'is an exon record whose strand (column 7) is not one of + - . ?'}
# the columns of an exon row, in the order the C entries of both scanners take them
_EXON_COLS = (('line', np.int64), ('chr_beg', np.int64), ('chr_len', np.int32), ('chr_hash', np.uint64), ('start', np.int64),
              ('end', np.int64), ('gene_beg', np.int64), ('gene_len', np.int32), ('gene_hash', np.uint64))
_C_TYPES = {np.int64: ctypes.c_int64, np.int32: ctypes.c_int32, np.uint64: ctypes.c_uint64}


def _exon_cols(cap):
    """Exon columns of `cap` rows for a C entry to fill: (dict of arrays, their pointers as arguments)."""
    cols = {k: np.empty(cap, dtype=t) for k, t in _EXON_COLS}
    return cols, [_lib._p(cols[k], _C_TYPES[t]) for k, t in _EXON_COLS]


def _error(err_line, err_kind):
    """(error line, error kind) of a C entry's two outputs, or None."""
    return (int(err_line.value), int(err_kind.value)) if err_kind.value else None


def _device(device):
    return int(os.environ.get('LOCAL_RANK', 0)) if device is None else int(device)


class Loader(object):

    def __init__(self, filetypes):
        """File loader for files that end with one of `filetypes` (a str or a list of str)."""
        self.filetypes = filetypes if isinstance(filetypes, list) else [filetypes]
        self.filename = None

    def get_file(self, to_load):
        if not isinstance(to_load, str):
            raise ValueError('{0} data type not understood'.format(to_load))
        if not os.path.exists(to_load):
            raise FileNotFoundError('file {0} not found'.format(to_load))
        if not any(to_load.endswith(ft) for ft in self.filetypes):
            raise ValueError('file {0} does not end with {1}'.format(to_load, ', '.join(self.filetypes)))
        self.filename = to_load

    def get_data(self):
        raise NotImplementedError('get_data not yet implemented for {0}'.format(self.__class__.__name__))


def _strand_col(cap, strand):
    """The strand column of `cap` rows for a _strand entry to fill, and its argument: ([array], [pointer]), or two empty lists."""
    col = [np.empty(cap, dtype=np.uint8)] if strand else []
    return col, [_lib._p(c, ctypes.c_uint8) for c in col]


def scan_window(buf, device=None, strand=False):
    """
    dn_gtf_scan on the bytes of one window: (number of lines, dict of the kept lines' columns -- `line` 1-based within the
    window, `chr_beg`, `chr_len`, `chr_hash`, `start`, `end`, `gene_beg`, `gene_len`, `gene_hash` -- (error line, error kind)
    or None, copy-in ms, device ms).  strand=True: dn_gtf_scan_strand, which adds the column `strand` (uint8: field seven of
    the line, one of + - . ?) and the error kind 4 for a field that is none of them.
    """
    lib = _lib.load()
    a = np.frombuffer(buf, dtype=np.uint8)
    cap = a.size // 20 + 1
    cols, col_args = _exon_cols(cap)
    i64 = ctypes.c_int64
    n_lines, n_rows, err_line, err_kind = i64(0), i64(0), i64(0), ctypes.c_int32(0)
    copy_ms, dev_ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
    s_col, s_arg = _strand_col(cap, strand)
    rc = (lib.dn_gtf_scan_strand if strand else lib.dn_gtf_scan)(
        _device(device), _lib._p(a, ctypes.c_uint8), a.size, cap, ctypes.byref(n_lines), ctypes.byref(n_rows),
        *(col_args + s_arg + [ctypes.byref(err_line), ctypes.byref(err_kind), ctypes.byref(copy_ms), ctypes.byref(dev_ms)]))
    _lib._check(rc, 'dn_gtf_scan')
    n = int(n_rows.value)
    cols.update(strand=s_col[0]) if strand else None
    return int(n_lines.value), {k: v[:n] for k, v in cols.items()}, _error(err_line, err_kind), float(copy_ms.value), float(dev_ms.value)


def _same_bytes(a, beg, other, length):
    """True when bytes a[beg[r] : beg[r] + length[r]] equal a[other[r] : other[r] + length[r]] for every row r."""
    width = int(length.max()) if length.size else 0
    if width == 0:
        return True
    step = max(_COMPARE_BYTES // width, 1)
    col = np.arange(width, dtype=np.int64)
    for lo in range(0, length.size, step):
        n = length[lo:lo + step, None]
        inside = col[None, :] < n
        x = a[np.where(inside, beg[lo:lo + step, None] + col, 0)]
        y = a[np.where(inside, other[lo:lo + step, None] + col, 0)]
        if not np.array_equal(x[inside], y[inside]):
            return False
    return True


def intern_spans(a, beg, length, hashes, table):
    """
    Codes of the byte spans a[beg : beg + length] in `table` ({bytes: code}, extended here): one bytes object per distinct
    span of the window.  Spans are grouped by hash; a group whose members differ (two names, one hash) sends the whole
    window through the dict one span at a time.
    """
    if beg.size == 0:
        return np.zeros(0, dtype=np.int64)
    _, first, inv = np.unique(hashes, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    rep = first[inv]
    if np.array_equal(length, length[rep]) and _same_bytes(a, beg, beg[rep], length):
        codes = np.empty(first.size, dtype=np.int64)
        for k in np.argsort(first).tolist():             # new names get their codes in order of first appearance
            r = int(first[k])
            codes[k] =table.setdefault(a[beg[r]:beg[r] + length[r]].tobytes(), len(table))
        return codes[inv]
    return np.array([table.setdefault(a[b:b + n].tobytes(), len(table)) for b, n in zip(beg.tolist(), length.tolist())],
                    dtype=np.int64)


def iter_windows(filename, window_bytes, device=None):
    """The file's bytes in pieces of about window_bytes that end at a line end (the last one at the end of the file).  The
    bytes of a .gz file are its inflated ones (gz.open_text: on GPU `device`, or with device=None by the host build)."""
    carry = b''
    with gz.open_text(filename, device=device) as f:
        while True:
            more = f.read(window_bytes)
            if not more:
                break
            cut = more.rfind(b'\n') + 1
            if cut == 0:                                  # a line longer than the window: keep reading
                carry += more
                continue
            head = more if cut == len(more) else more[:cut]
            yield carry + head if carry else head
            carry = more[cut:]
    if carry:
        yield carry


class GeneAnnotationLoader(Loader):
    FILETYPES = ['.gtf', '.gtf.gz']

    def __init__(self, to_load, window_bytes=None, device=None):
        """
        .gtf file loader on the device.

        :param to_load: str the realpath to a file that ends with FILETYPES.
        :param window_bytes: the file is uploaded and scanned in windows of about this many bytes, cut at line ends (default
        WINDOW_BYTES); the table and the errors do not depend on it.
        :param device: HIP device index (default: LOCAL_RANK or 0).
        """
        Loader.__init__(self, self.FILETYPES)
        self.get_file(to_load)
        self.window_bytes = max(int(WINDOW_BYTES if window_bytes is None else window_bytes), 1)
        self.device = device
        self.timing = {}

    def exon_codes(self, strand=False):
        """
        The exon lines of the file in file order, names as codes: (chr code, start, end, gene code -- int64 arrays --,
        chromosome names, gene names: lists of str indexed by code, in order of first appearance).  strand=True: a seventh
        entry, the strand byte of every line (uint8: + - . ?).
        """
        chr_table, gene_table = {}, {}
        parts = []
        line_base = 0
        t = self.timing = {'read_s': 0.0, 'copy_ms': 0.0, 'device_ms': 0.0, 'bytes': 0}
        t0 = time.perf_counter()
        for win in iter_windows(self.filename, self.window_bytes, _device(self.device)):
            t['read_s'] += time.perf_counter() - t0
            n_lines, cols, err, copy_ms, dev_ms = scan_window(win, self.device, strand)
            t['copy_ms'] += copy_ms
            t['device_ms'] += dev_ms
            t['bytes'] += len(win)
            if err is not None:
                raise ValueError('File {0}, line {1} {2}'.format(self.filename, line_base + err[0], _KINDS[err[1]]))
            a = np.frombuffer(win, dtype=np.uint8)
            parts.append((intern_spans(a, cols['chr_beg'], cols['chr_len'].astype(np.int64), cols['chr_hash'], chr_table),
                          cols['start'], cols['end'],
                          intern_spans(a, cols['gene_beg'], cols['gene_len'].astype(np.int64), cols['gene_hash'], gene_table),
                          cols['strand'] if strand else None))
            line_base += n_lines
            t0 = time.perf_counter()
        t['read_s'] += time.perf_counter() - t0
        t['lines'] = line_base
        cat = [np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=np.int64) for k in range(4)]
        names = [[b.decode('utf-8', 'replace') for b in tab] for tab in (chr_table, gene_table)]     # dicts keep insertion order
        if strand:
            return cat[0], cat[1], cat[2], cat[3], names[0], names[1], np.concatenate([p[4] for p in parts]) if parts else np.zeros(0, np.uint8)
        return cat[0], cat[1], cat[2], cat[3], names[0], names[1]

    def get_data(self, strand=False):
        """
        The reference's exon table (loaders.py:114-168): columns `chr` (str), `start` (int64), `end` (int64), `gene` (str),
        one row per exon line of the file, duplicates of the four columns dropped (the first one stays), RangeIndex.
        Malformed input raises ValueError naming the file, the line and what is wrong with it.
        strand=True (strand-specific counting): a fifth column `strand`, field seven of the exon line itself, '+', '-', '.'
        or '?'; any other field is then a malformed line.  Duplicates are rows equal in all five columns.
        """
        from pandas import DataFrame
        codes = self.exon_codes(strand)
        chr_code, start, end, gene_code, chr_names, gene_names = codes[:6]
        cols = {'chr': chr_code, 'start': start, 'end': end, 'gene': gene_code}
        if strand:
            cols['strand'] = codes[6]
        keep = ~DataFrame(cols).duplicated().values
        out = {'chr': np.array(chr_names, dtype=object)[chr_code[keep]] if chr_names else np.zeros(0, dtype=object),
               'start': start[keep].astype(np.int64), 'end': end[keep].astype(np.int64),
               'gene': np.array(gene_names, dtype=object)[gene_code[keep]] if gene_names else np.zeros(0, dtype=object)}
        if strand:
            out['strand'] = np.array([chr(c) for c in range(128)], dtype=object)[codes[6][keep]]
        return DataFrame(out)


class Gff3Scan(object):
    """
    One load of a GFF3 text of total_bytes on the device (dn_gff3_open ... dn_gff3_close): `window(buf)` for every piece of the
    text in order, each ending at a line end, then `resolve()`; use as a context manager.  `pending` collects the exon rows that
    named a Parent: (row index among all rows so far, line, parent span and hash).
    """

    def __init__(self, total_bytes, device=None, hash_bits=64):
        self.lib = _lib.load()
        self.h = ctypes.c_void_p(None)
        _lib._check(self.lib.dn_gff3_open(_device(device), int(total_bytes), int(hash_bits), ctypes.byref(self.h)), 'dn_gff3_open')
        self.lines, self.fasta_line, self.nodes = 0, 0, 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.h:
            self.lib.dn_gff3_close(self.h)
            self.h = ctypes.c_void_p(None)

    def window(self, buf, strand=False):
        """
        dn_gff3_window on the next piece of the text: (dict of the exon rows' columns -- `line` 1-based in the file, spans as
        offsets in the file, `pending` 1 where gene_* is a Parent still to resolve --, (error line, error kind) or None,
        copy-in ms, device ms).  self.fasta_line becomes the line of `##FASTA` once a window held it: feed no more then.
        strand=True: dn_gff3_window_strand, which adds the column `strand` (uint8: field seven of the exon line) and error kind 6.
        """
        a = np.frombuffer(buf, dtype=np.uint8)
        cap = a.size // 20 + 1
        cols, col_args = _exon_cols(cap)
        pending = np.empty(cap, dtype=np.uint8)
        i64 = ctypes.c_int64
        n_lines, n_rows, fasta, err_line, err_kind = i64(0), i64(0), i64(0), i64(0), ctypes.c_int32(0)
        copy_ms, dev_ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
        s_col, s_arg = _strand_col(cap, strand)
        rc = (self.lib.dn_gff3_window_strand if strand else self.lib.dn_gff3_window)(
            self.h, _lib._p(a, ctypes.c_uint8), a.size, cap, ctypes.byref(n_lines), ctypes.byref(n_rows),
            *(col_args + [_lib._p(pending, ctypes.c_uint8)] + s_arg + [ctypes.byref(fasta), ctypes.byref(err_line),
                                                                       ctypes.byref(err_kind), ctypes.byref(copy_ms), ctypes.byref(dev_ms)]))
        _lib._check(rc, 'dn_gff3_window')
        n = int(n_rows.value)
        self.lines += int(n_lines.value)
        self.fasta_line = int(fasta.value)
        cols = {k: v[:n] for k, v in cols.items()}
        cols['pending'] = pending[:n]
        if strand:
            cols['strand'] = s_col[0][:n]
        return cols, _error(err_line, err_kind), float(copy_ms.value), float(dev_ms.value)

    def resolve(self, line, par_beg, par_len, par_hash):
        """dn_gff3_resolve: (name_beg, name_len, name_hash of every pending row, (error line, kind) or None, ms)."""
        n = int(line.size)
        line, par_beg = np.ascontiguousarray(line, dtype=np.int64), np.ascontiguousarray(par_beg, dtype=np.int64)
        par_len, par_hash = np.ascontiguousarray(par_len, dtype=np.int32), np.ascontiguousarray(par_hash, dtype=np.uint64)
        out = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint64)
        i64, i32, u64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64
        n_nodes, err_line, err_kind, ms = i64(0), i64(0), i32(0), ctypes.c_double(0.0)
        rc = self.lib.dn_gff3_resolve(self.h, n, _lib._p(line, i64), _lib._p(par_beg, i64), _lib._p(par_len, i32), _lib._p(par_hash, u64),
                                      _lib._p(out[0], i64), _lib._p(out[1], i32), _lib._p(out[2], u64), ctypes.byref(n_nodes),
                                      ctypes.byref(err_line), ctypes.byref(err_kind), ctypes.byref(ms))
        _lib._check(rc, 'dn_gff3_resolve')
        self.nodes = int(n_nodes.value)
        return out[0], out[1], out[2], _error(err_line, err_kind), float(ms.value)


def _resolve_pending(scan, cols):
    """The rows `cols` (all windows, concatenated) with the names of the pending ones filled in by scan.resolve: (error or
    None, resolve ms, number of pending rows)."""
    idx = np.flatnonzero(cols['pending'])
    nb, nl, nh, err, ms = scan.resolve(cols['line'][idx], cols['gene_beg'][idx], cols['gene_len'][idx], cols['gene_hash'][idx])
    if err is None:
        cols['gene_beg'][idx], cols['gene_len'][idx], cols['gene_hash'][idx] = nb, nl, nh
    return err, ms, int(idx.size)


def gff3_scan(data, device=None, hash_bits=64, stats=None, strand=False):
    """
    The GFF3 rule on the bytes of a whole annotation: (number of lines, dict of the exon rows' columns in file order -- `line`
    1-based, `chr_beg`, `chr_len`, `chr_hash`, `start`, `end`, and `gene_beg`, `gene_len`, `gene_hash` of the resolved gene
    name --, (error line, error kind) or None; with an error there are no rows).  device=None runs the host build
    (dn_gff3_scan_host), a device index the device build as one window.  hash_bits masks the hashes of IDs and Parents in
    both builds: with few bits many IDs share a hash, and the result must not change.  stats (dict): `nodes`, `walked_exons`.
    strand=True: the _strand entries of both builds, which add the column `strand` (uint8: field seven of the exon line, one of
    + - . ?) and the error kind 6 for an exon line whose field is none of them.
    """
    a = np.frombuffer(data, dtype=np.uint8)
    stats = {} if stats is None else stats
    if a.size == 0:
        stats.update(nodes=0, walked_exons=0)
        return 0, dict(_exon_cols(0)[0], **({'strand': np.zeros(0, np.uint8)} if strand else {})), None
    if device is None:
        lib = _lib.load()
        cap = a.size // 20 + 1
        cols, col_args = _exon_cols(cap)
        i64 = ctypes.c_int64
        n_lines, n_rows, n_nodes, n_walked, err_line, err_kind = i64(0), i64(0), i64(0), i64(0), i64(0), ctypes.c_int32(0)
        s_col, s_arg = _strand_col(cap, strand)
        rc = (lib.dn_gff3_scan_host_strand if strand else lib.dn_gff3_scan_host)(
            _lib._p(a, ctypes.c_uint8), a.size, int(hash_bits), cap, ctypes.byref(n_lines), ctypes.byref(n_rows),
            *(col_args + s_arg + [ctypes.byref(n_nodes), ctypes.byref(n_walked), ctypes.byref(err_line), ctypes.byref(err_kind)]))
        _lib._check(rc, 'dn_gff3_scan_host')
        cols.update(strand=s_col[0]) if strand else None
        stats.update(nodes=int(n_nodes.value), walked_exons=int(n_walked.value))
        return int(n_lines.value), {k: v[:int(n_rows.value)] for k, v in cols.items()}, _error(err_line, err_kind)
    with Gff3Scan(a.size, device, hash_bits) as scan:
        cols, err, _, _ = scan.window(a, strand)
        walked = 0
        if err is None:
            err, _, walked = _resolve_pending(scan, cols)
        stats.update(nodes=scan.nodes, walked_exons=walked)
        if err is not None:
            cols = {k: v[:0] for k, v in cols.items()}
        cols.pop('pending')
        return scan.lines, cols, err


class Gff3AnnotationLoader(GeneAnnotationLoader):
    """.gff3 / .gff file loader on the device (a .gff file is read as GFF3): the constructor and the table of GeneAnnotationLoader."""
    FILETYPES = ['.gff3', '.gff', '.gff3.gz', '.gff.gz']

    def _raise(self, err):
        raise ValueError('File {0}, line {1} {2}'.format(self.filename, err[0], _GFF3_KINDS[err[1]]))

    def exon_codes(self, strand=False):
        """As GeneAnnotationLoader.exon_codes.  The text stays on the device until every exon has its gene."""
        t = self.timing = {'read_s': 0.0, 'copy_ms': 0.0, 'device_ms': 0.0, 'resolve_ms': 0.0, 'bytes': 0, 'lines': 0, 'nodes': 0,
                           'walked_exons': 0}
        zipped = gz.is_gz(self.filename)             # the text's size: from a first scan of the .gz file, not from its ISIZE
        size = gz.inflated_size(self.filename, _device(self.device)) if zipped else os.path.getsize(self.filename)
        empty = np.zeros(0, dtype=np.int64)
        none = (empty, empty, empty, empty, [], []) + ((np.zeros(0, np.uint8),) if strand else ())
        if size == 0:
            return none
        parts, text = [], []
        with Gff3Scan(size, self.device) as scan:
            t0 = time.perf_counter()
            for win in iter_windows(self.filename, self.window_bytes, _device(self.device)):
                t['read_s'] += time.perf_counter() - t0
                if zipped:
                    text.append(win)
                cols, err, copy_ms, dev_ms = scan.window(win, strand)
                t['copy_ms'] += copy_ms
                t['device_ms'] += dev_ms
                t['bytes'] += len(win)
                if err is not None:
                    self._raise(err)
                parts.append(cols)
                t0 = time.perf_counter()
                if scan.fasta_line:
                    break
            t['read_s'] += time.perf_counter() - t0
            t['lines'] = scan.lines
            cols = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]} if parts else None
            if cols is None or cols['line'].size == 0:
                return none
            err, t['resolve_ms'], t['walked_exons'] = _resolve_pending(scan, cols)
            t['nodes'] = scan.nodes
            if err is not None:
                self._raise(err)
        a = np.frombuffer(b''.join(text), dtype=np.uint8) if zipped else np.memmap(self.filename, dtype=np.uint8, mode='r')
        chr_table, gene_table = {}, {}
        chr_code = intern_spans(a, cols['chr_beg'], cols['chr_len'].astype(np.int64), cols['chr_hash'], chr_table)
        gene_code = intern_spans(a, cols['gene_beg'], cols['gene_len'].astype(np.int64), cols['gene_hash'], gene_table)
        names = [[b.decode('utf-8', 'replace') for b in tab] for tab in (chr_table, gene_table)]
        return (chr_code, cols['start'], cols['end'], gene_code, names[0], names[1]) + ((cols['strand'],) if strand else ())


ANNOTATION_LOADERS = (('.gtf', GeneAnnotationLoader), ('.gff3', Gff3AnnotationLoader), ('.gff', Gff3AnnotationLoader),
                      ('.gtf.gz', GeneAnnotationLoader), ('.gff3.gz', Gff3AnnotationLoader), ('.gff.gz', Gff3AnnotationLoader))


def annotation_loader(path, **kw):
    """The loader of an annotation file by its extension: .gtf -> GeneAnnotationLoader, .gff3 / .gff -> Gff3AnnotationLoader;
    the same with a further .gz (gz.open_text inflates it)."""
    if isinstance(path, str):
        for ext, cls in ANNOTATION_LOADERS:
            if path.endswith(ext):
                return cls(path, **kw)
    loader = Loader([ext for ext, _ in ANNOTATION_LOADERS])
    loader.get_file(path)                            # raises: data type, file not found, or "does not end with"
    raise ValueError('file {0} does not end with {1}'.format(path, ', '.join(loader.filetypes)))

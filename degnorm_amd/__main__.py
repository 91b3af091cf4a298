"""
`python -m degnorm_amd`: the `degnorm` command on the MI355X (reference: `degnorm/__main__.py`, `degnorm/utils.py:195-484`).

    python -m degnorm_amd --bam-files s1.bam s2.bam -g genes.gtf -o out [--iter 5 --nmf-iter 100 -d 1 ...]
    python -m degnorm_amd --bam-dir DIR -g genes.gtf -o out
    python -m degnorm_amd -w PREVIOUS_OUTPUT_DIR -o out

    python -m degnorm_amd --bam-dir DIR --create-bai -g genes.gtf -o out
    python -m degnorm_amd --bam-dir DIR --sort-bam -g genes.gtf -o out
    python -m degnorm_amd --sam-files s1.sam s2.sam -g genes.gtf -o out
    python -m degnorm_amd --sam-dir DIR -g genes.gtf -o out

The flags and their validation follow the reference.  With --create-bai a .bam file without a .bai file next to it gets
one before the run (the reference shells out to samtools for this; here degnorm_amd.bam.create_index builds it on the GPU);
without the flag a missing index is an error.  A .bai index ends at position 2^29: --index-format csi has every index the
command creates written as X.csi, and where X.bai is missing an X.csi or X.bam.csi that lies there is read.
With --sort-bam every .bam file whose header does not say SO:coordinate -- an aligner's unsorted or name-collated output -- is first sorted by coordinate on the GPU (degnorm_amd.bam.sort_bam; the
reference's documentation runs samtools sort for this) to <output directory>/sorted_bam/<the same file name>, indexed
there, and read in place of the input; the sorted copies are kept, and files that say SO:coordinate are used as they are.
With --sam-files / --sam-dir the inputs are SAM text, what HISAT2, Bowtie2, BWA and (by default) STAR write: every X.sam is
first converted on the GPU (degnorm_amd.bam.sam_to_bam; the reference's documentation runs samtools view -b for this) to
<output directory>/converted_bam/X.bam and from there treated as a --sort-bam input: sorted to sorted_bam/ and indexed there
when its header does not say SO:coordinate, indexed where it lies when it does.  No samtools step is left.
--pair-by flag pairs mates by FLAG (0x1, 0x40, 0x80) and mate position, what those aligners write: both mates of a template
carry one name there, and the default --pair-by name (the reference's .1 / .2 suffixes) takes such a file for single-end.
--pair-by auto tries the names first.  --exclude-flags, --require-flags (decimal or 0x...) and --min-mapq drop records as
samtools view -F / -f / -q does; they work on --bam-* inputs and on --sam-* / --sort-bam ones, whose converted and sorted
copies keep FLAG, MAPQ and PNEXT.
--stranded forward | reverse counts reads by strand (stranded libraries; reverse is dUTP / TruSeq Stranded): every gene with
the reads of its own strand only, opposite-strand genes on the same bases apart; it reaches the same inputs.
Annotations and SAM text may be gzip-compressed (genes.gtf.gz, genes.gff3.gz, X.sam.gz): degnorm_amd.gz inflates them on the GPU.
Not offered: SAM output, gzip output, zstd, bzip2 and .Z input, --plot-genes, the HTML report and the MPI command (see
degnorm_amd.warm_start --mpi for the sharded NMF-OA run).  Raw and estimated coverage curves of an output directory as text
files: `python -m degnorm_amd.data_access -d OUTPUT_DIR -g GENE [GENE ...] | all -o SAVE_DIR` (the reference's
get_coverage_data; its get_coverage_plots is not offered).
"""
import argparse
import logging
import os
import re
import sys
from datetime import datetime


def _flag_mask(text):
    """A FLAG mask of the command line: decimal, or hexadecimal with 0x in front."""
    try:
        return int(text, 16 if text.lower().startswith('0x') else 10)
    except ValueError:
        raise argparse.ArgumentTypeError('{0!r} is not a decimal or 0x... number'.format(text))


def argparser():
    ap = argparse.ArgumentParser(
        prog='python -m degnorm_amd',
        description='DegNorm (RNA-seq degradation normalization) from .bam and .gtf / .gff3 files on an AMD Instinct GPU.',
        epilog='Not available in this command: --plot-genes, the HTML summary report and the MPI command; coverage curves of an output '
               'directory are written as text by `python -m degnorm_amd.data_access` (plots are not offered).  A .bam file must be '
               'sorted by coordinate and needs its .bai index file: --sort-bam sorts (and indexes) the files that are not sorted, '
               '--create-bai makes the missing index files of sorted ones.  Alignments in SAM text need none of this: '
               '--sam-files / --sam-dir convert, sort and index them.')
    ap.add_argument('--bam-files', nargs='+', default=None,
                    help='sorted .bam alignment files, one per sample (single-end or paired), at least two')
    ap.add_argument('--bai-files', nargs='+', default=None,
                    help='.bai (or .csi) index files in the order of --bam-files; without this flag every X.bam needs X.bai (or, '
                         'without one, X.csi or X.bam.csi) next to it')
    ap.add_argument('--bam-dir', default=None,
                    help='directory whose .bam files (with .bai files of the same base name) are the input; '
                         'not together with --bam-files / --bai-files')
    ap.add_argument('--sam-files', nargs='+', default=None,
                    help='.sam alignment files (an aligner\'s text output), one per sample, at least two: each is converted on the '
                         'GPU to <output directory>/converted_bam/<name>.bam, sorted to sorted_bam/ unless its header says '
                         'SO:coordinate, and indexed; not together with --bam-files, --bam-dir, --bai-files or -w')
    ap.add_argument('--sam-dir', default=None,
                    help='directory whose .sam files are the input, as with --sam-files; not together with --sam-files')
    ap.add_argument('-w', '--warm-start-dir', default=None,
                    help='output directory of an earlier run: reuse its coverage matrices, read counts and gene table and '
                         'skip the alignment and annotation stages (.bam / annotation arguments are then ignored)')
    ap.add_argument('-g', '--genome-annotation', type=str, default=None,
                    help='.gtf, .gff3 or .gff (read as GFF3) annotation file, optionally gzip-compressed (.gtf.gz ...); required unless -w is given')
    ap.add_argument('-o', '--output-dir', type=str, default=None,
                    help='output directory: created when it does not exist; inside an existing directory, or without this '
                         'flag in the working directory, a degnorm_<mmddYYYY>_<HHMMSS> directory is created')
    ap.add_argument('-d', '--downsample-rate', type=int, default=1,
                    help='fit every gene on each d-th base of its transcript (default 1: all bases)')
    ap.add_argument('--nmf-iter', type=int, default=100, help='iterations of one NMF-OA factorisation (default 100)')
    ap.add_argument('--iter', type=int, default=5, help='DegNorm iterations (default 5)')
    ap.add_argument('--minimax-coverage', type=int, default=0,
                    help='leave out genes whose highest coverage over all samples is below this (default 0)')
    ap.add_argument('-s', '--skip-baseline-selection', action='store_true', help='do not run baseline selection')
    ap.add_argument('--non-unique-alignments', action='store_true',
                    help='keep reads flagged NH > 1 (by default only uniquely aligned reads count)')
    ap.add_argument('-p', '--proc-per-node', type=int, default=1,
                    help='host threads for reading .bam files and packing genes (default 1)')
    ap.add_argument('--create-bai', action='store_true',
                    help='create the .bai index file X.bai of every X.bam that has none next to it, on the GPU, before the run '
                         '(not with --bai-files)')
    ap.add_argument('--index-format', choices=('bai', 'csi'), default='bai',
                    help='the format of every index file this command creates (--create-bai, and the sorted copies of --sort-bam, '
                         '--sam-files and --sam-dir): bai (the default), or csi, which a reference of more than 2^29 bases needs; '
                         'X.csi is written in place of X.bai')
    ap.add_argument('--sort-bam', action='store_true',
                    help='sort every .bam file whose header does not say SO:coordinate by coordinate, on the GPU, to '
                         '<output directory>/sorted_bam/<same name>, index the sorted copy there and use it in place of the '
                         'input; the copies are kept (not with --bai-files)')
    ap.add_argument('--native-deflate', action='store_true',
                    help='with --sort-bam, --sam-files or --sam-dir: deflate the blocks of the converted and sorted copies on the '
                         'GPU with the library\'s own encoder instead of with zlib on the host')
    ap.add_argument('--device-inflate', action='store_true',
                    help='inflate the BGZF blocks of the .bam files on the GPU instead of with zlib on the host')
    ap.add_argument('--device-frame', action='store_true',
                    help='find the record starts of the inflated .bam bytes on the GPU instead of with a serial walk on the host')
    ap.add_argument('--device-pair', action='store_true',
                    help='pair the mates of paired-end .bam files on the GPU instead of with a sort of their names on the host; '
                         'reads of equal name keep their order in the file')
    ap.add_argument('--pair-by', choices=('name', 'flag', 'auto'), default='name',
                    help='how paired-end files are recognised and their mates told: name (the default) -- read names that end in '
                         '.1 / .2, mates share the name before that suffix; flag -- FLAG 0x1 / 0x40 / 0x80 and the mate position, '
                         'what HISAT2, STAR, BWA and Bowtie2 write (always paired on the GPU); auto -- name if the names say '
                         'paired, otherwise flag')
    ap.add_argument('--exclude-flags', type=_flag_mask, default=0, metavar='MASK',
                    help='drop every record that has one of these FLAG bits set, as samtools view -F (decimal or 0x...; e.g. 0x904 '
                         'for unmapped, secondary and supplementary records; default 0)')
    ap.add_argument('--require-flags', type=_flag_mask, default=0, metavar='MASK',
                    help='drop every record that lacks one of these FLAG bits, as samtools view -f (decimal or 0x...; default 0)')
    ap.add_argument('--min-mapq', type=int, default=0, help='drop every record whose MAPQ is below this, as samtools view -q (0 .. 255; default 0)')
    ap.add_argument('--stranded', choices=('no', 'forward', 'reverse'), default='no',
                    help='count reads by strand, for stranded libraries: forward -- a single read or first mate lies on the strand '
                         'of its gene (htseq-count -s yes, featureCounts -s 1); reverse -- on the opposite strand, dUTP / TruSeq Stranded '
                         '(-s reverse, -s 2).  Genes without a single strand in the annotation are left out; no (the default) counts '
                         'every read as if the library were unstranded')
    ap.add_argument('--verify-crc', action='store_true',
                    help='check every BGZF block read from the .bam files against the CRC32 of its trailer (also while '
                         '--create-bai indexes and --sort-bam sorts them) and stop at the first that differs')
    return ap


def bai_from_bam_file(bam_file):
    if not bam_file.endswith('.bam'):
        raise ValueError('{0} must have a .bam extension.'.format(bam_file))
    return bam_file[:-3] + 'bai'


def _default_bai_files(bam_files, create=False, sort=(), fmt='bai'):
    """(X.bai of every X.bam, the .bam files whose X.bai is missing); without `create` a missing one is an error.  Where
    X.bai is missing, X.csi and then X.bam.csi are taken; an index that is created is X.<fmt>.  The files of `sort` are
    sorted and indexed later: their entry is None."""
    bai_files, create_bai_files = [], []
    for bam_file in bam_files:
        if bam_file in sort:
            bai_files.append(None)
            continue
        bai_file = re.sub('.bam$', '.bai', bam_file)
        if not os.path.isfile(bai_file):
            csi_files = [f for f in (re.sub('.bam$', '.csi', bam_file), bam_file + '.csi') if os.path.isfile(f)]
            if csi_files:
                bai_files.append(csi_files[0])
                continue
            if not create:
                raise FileNotFoundError('No .bai index file {0} for {1}: pass --create-bai to have it made, index the .bam file '
                                        'first (e.g. samtools index), or name the index files with --bai-files.'
                                        .format(bai_from_bam_file(bam_file), bam_file))
            bai_file = bai_from_bam_file(bam_file)[:-3] + fmt
            create_bai_files.append(bam_file)
        bai_files.append(bai_file)
    return bai_files, create_bai_files


def _unsorted(bam_files):
    """The .bam files whose header does not say SO:coordinate."""
    from .bam import sort_order
    return [b for b in bam_files if sort_order(b) != 'coordinate']


def _sam_inputs(args):
    """The .sam and .sam.gz files of --sam-files / --sam-dir, checked: a list of at least two existing files with unique base names."""
    from .gz import is_gz, strip_gz
    if args.bam_files or args.bam_dir or args.bai_files is not None or args.warm_start_dir:
        raise ValueError('Do not specify --sam-files or --sam-dir together with --bam-files, --bam-dir, --bai-files or --warm-start-dir.')
    if args.sam_files and args.sam_dir:
        raise ValueError('Do not specify both --sam-files and --sam-dir. Use one input selection method or the other.')
    if args.sam_dir:
        if not os.path.isdir(args.sam_dir):
            raise NotADirectoryError('Cannot find --sam-dir {0}'.format(args.sam_dir))
        sam_files = [os.path.join(args.sam_dir, f) for f in sorted(os.listdir(args.sam_dir)) if strip_gz(f).endswith('.sam')]
        for f in sam_files:
            if is_gz(f) and strip_gz(f) in sam_files:
                raise ValueError('{0} and {1} would both become {2}.bam: keep one of them.'.format(strip_gz(f), f, os.path.basename(f)[:-7]))
        if len(sam_files) < 2:
            raise ValueError('Only found {0} .sam files within directory {1}'.format(len(sam_files), args.sam_dir))
    else:
        sam_files = list(args.sam_files)
        for sam_file in sam_files:
            if not strip_gz(sam_file).endswith('.sam'):
                raise ValueError('{0} is not a .sam file. (X.sam or X.sam.gz is expected.)'.format(sam_file))
            if not os.path.isfile(sam_file):
                raise FileNotFoundError('Could not find .sam file {0}'.format(sam_file))
    if len(sam_files) < 2:
        raise ValueError('Fewer than 2 .sam files were found. Not sufficiently many to run DegNorm.')
    if len(set(os.path.basename(strip_gz(f)) for f in sam_files)) != len(sam_files):
        raise ValueError('The .sam files are not uniquely named: their converted copies share one directory.')
    return sam_files


def validate_args(args):
    """The reference's checks on parsed arguments (utils.py:338-482); fills args.bam_files / args.bai_files, and
    args.create_bai_files with the .bam files whose index is to be made first (empty without args.create_bai) and
    args.sort_bam_files with those that are to be sorted first (empty without args.sort_bam; their index file is None).
    With --sam-files / --sam-dir args.sam_files is the checked list of .sam files and the .bam lists are empty: _run fills them
    as it converts."""
    create = getattr(args, 'create_bai', False)
    sort = getattr(args, 'sort_bam', False)
    fmt = args.index_format = getattr(args, 'index_format', 'bai')
    args.sort_bam_files = []
    args.sam_files, args.sam_dir = getattr(args, 'sam_files', None), getattr(args, 'sam_dir', None)
    sam = bool(args.sam_files or args.sam_dir)
    if sort and args.bai_files is not None:
        raise ValueError('Do not specify both --sort-bam and --bai-files: a sorted copy gets an index file of its own.')
    if getattr(args, 'native_deflate', False) and not sort and not sam:
        raise ValueError('Do not specify --native-deflate without --sort-bam: it chooses the encoder of the sorted copies.')
    if sam:
        args.sam_files = _sam_inputs(args)
    if (not args.bam_files and not args.bam_dir) and (not args.warm_start_dir) and not sam:
        raise ValueError('Must specify either --bam-files, --bam-dir, or --warm-start-dir as a data input option.')
    n_cpu = os.cpu_count() or 1
    if args.proc_per_node > n_cpu:
        logging.warning('{0} is greater than the number of available cores ({1}). Reducing to {2}.'
                        .format(args.proc_per_node, n_cpu, max(n_cpu - 1, 1)))
        args.proc_per_node = max(n_cpu - 1, 1)
    if not args.warm_start_dir:
        from .bam import check_read_options
        from .reads import check_stranded
        check_read_options(getattr(args, 'pair_by', 'name'), getattr(args, 'exclude_flags', 0), getattr(args, 'require_flags', 0),
                           getattr(args, 'min_mapq', 0))
        check_stranded(getattr(args, 'stranded', 'no'))
    if (args.nmf_iter < 1) or (args.iter < 1) or (args.downsample_rate < 1):
        raise ValueError('--nmf-iter, --iter, and --downsample-rate must all be >= 1.')
    if args.warm_start_dir:
        if not os.path.isdir(args.warm_start_dir):
            raise NotADirectoryError('Cannot find --warm-start-dir {0}'.format(args.warm_start_dir))
        if args.bam_files or args.bam_dir or args.genome_annotation:
            logging.warning('Using warm-start directory. Supplied .bam files, .bam directory, '
                            'and genome annotation file will be ignored.')
        args.bam_files = args.bai_files = args.bam_dir = args.genome_annotation = None
        args.create_bai_files = None
        return args
    if not args.genome_annotation:
        raise ValueError('If warm-start directory not specified, gene annotation file must be specified!')
    if not os.path.isfile(args.genome_annotation):
        raise FileNotFoundError('Gene annotation file {0} not found.'.format(args.genome_annotation))
    bam_files, bai_files, create_bai_files = [], [], []
    if sam:
        args.bam_files, args.bai_files, args.create_bai_files = [], [], []
        return args
    if args.bam_dir:
        if args.bam_files is not None or args.bai_files is not None:
            raise ValueError('Do not specify both a --bam-dir and either --bam-files and/or --bai-files.'
                             'Use one input selection method or the other.')
        if not os.path.isdir(args.bam_dir):
            raise NotADirectoryError('Cannot find --bam-dir {0}'.format(args.bam_dir))
        bam_files = [os.path.join(args.bam_dir, f) for f in sorted(os.listdir(args.bam_dir)) if f.endswith('.bam')]
        if len(bam_files) < 2:
            raise ValueError('Only found {0} .bam files within directory {1}'.format(len(bam_files), args.bam_dir))
        bai_files, create_bai_files = _default_bai_files(bam_files, create, _unsorted(bam_files) if sort else (), fmt)
    else:
        for bam_file in args.bam_files:
            if not bam_file.endswith('.bam'):
                raise ValueError('{0} is not a .bam file.'.format(bam_file))
            if not os.path.isfile(bam_file):
                raise FileNotFoundError('Count not find .bam file {0}'.format(bam_file))
            bam_files.append(bam_file)
        if args.bai_files is not None:
            if len(args.bai_files) != len(bam_files):
                raise ValueError('Number of supplied .bai files does not match number of supplied .bam files.')
            for bai_file in args.bai_files:
                if not bai_file.endswith(('.bai', '.csi')):
                    raise ValueError('{0} is not a .bai file.'.format(bai_file))
                if not os.path.isfile(bai_file):
                    raise FileNotFoundError('Count not find .bai file {0}'.format(bai_file))
                bai_files.append(bai_file)
        else:
            bai_files, create_bai_files = _default_bai_files(bam_files, create, _unsorted(bam_files) if sort else (), fmt)
    if len(bam_files) < 2:
        raise ValueError('Fewer than 2 .bam files were found. Not sufficiently many to run DegNorm.')
    if len(bam_files) != len(set(bam_files)):
        raise ValueError('Supplied .bam files are not uniquely named!')
    args.bam_files, args.bai_files, args.create_bai_files = bam_files, bai_files, create_bai_files
    args.sort_bam_files = [b for b, i in zip(bam_files, bai_files) if i is None]
    if len(set(os.path.basename(b) for b in args.sort_bam_files)) != len(args.sort_bam_files):
        raise ValueError('The .bam files to be sorted are not uniquely named: their sorted copies share one directory.')
    return args


def create_output_dir(user_input=None):
    """
    The output directory (created when missing), by the reference's three rules (utils.py:49-79): none given ->
    ./degnorm_<mmddYYYY>_<HHMMSS>; an existing path -> <path>/degnorm_<mmddYYYY>_<HHMMSS>; otherwise the path itself, in the
    working directory when it is a bare name.
    """
    stamp = 'degnorm_' + datetime.now().strftime('%m%d%Y_%H%M%S')
    if not user_input:
        output_dir = os.path.join(os.getcwd(), stamp)
    elif os.path.exists(user_input):
        output_dir = os.path.join(user_input, stamp)
    else:
        output_dir = user_input
        if os.path.dirname(user_input) == '':
            output_dir = os.path.join(os.getcwd(), user_input)
    if not os.path.exists(output_dir):
        os.makedirs(output_dir)
    return output_dir


def _run(args, output_dir, device, verify):
    logging.info('DegNorm output directory -- {0}'.format(output_dir))
    if args.warm_start_dir:
        from .warm_start import run_from_warm_start
        logging.info('WARM-START: loading data from previous DegNorm run contained in {0}'.format(args.warm_start_dir))
        run_from_warm_start(args.warm_start_dir, output_dir, degnorm_iter=args.iter, nmf_iter=args.nmf_iter,
                            downsample_rate=args.downsample_rate, skip_baseline_selection=args.skip_baseline_selection,
                            minimax_coverage=args.minimax_coverage)
    else:
        from .pipeline import run_pipeline
        deflate = 'native' if getattr(args, 'native_deflate', False) else 'zlib'
        fmt = getattr(args, 'index_format', 'bai')
        for k, sam_file in enumerate(getattr(args, 'sam_files', None) or []):
            from .bam import create_index, sam_to_bam, sort_order
            from .gz import strip_gz
            converted_dir = os.path.join(output_dir, 'converted_bam')
            os.makedirs(converted_dir, exist_ok=True)
            logging.info('converting {0} to BAM -- {1} / {2}'.format(sam_file, k + 1, len(args.sam_files)))
            bam_file = sam_to_bam(sam_file, os.path.join(converted_dir, os.path.basename(strip_gz(sam_file))[:-4] + '.bam'), device=device,
                                  n_jobs=args.proc_per_node, deflate=deflate)
            args.bam_files.append(bam_file)
            if sort_order(bam_file) != 'coordinate':
                args.bai_files.append(None)
                args.sort_bam_files.append(bam_file)
            else:
                args.bai_files.append(create_index(bam_file, bai_from_bam_file(bam_file)[:-3] + fmt, device=device, verify=verify, fmt=fmt))
        for k, bam_file in enumerate(args.sort_bam_files):
            from .bam import create_index, sort_bam
            sorted_dir = os.path.join(output_dir, 'sorted_bam')
            os.makedirs(sorted_dir, exist_ok=True)
            logging.info('sorting {0} by coordinate -- {1} / {2}'.format(bam_file, k + 1, len(args.sort_bam_files)))
            at = args.bam_files.index(bam_file)
            args.bam_files[at] = sort_bam(bam_file, os.path.join(sorted_dir, os.path.basename(bam_file)), device=device,
                                          n_jobs=args.proc_per_node, verify=verify, deflate=deflate)
            args.bai_files[at] = create_index(args.bam_files[at], bai_from_bam_file(args.bam_files[at])[:-3] + fmt, device=device,
                                              verify=verify, fmt=fmt)
        run_pipeline(args.bam_files, args.bai_files, args.genome_annotation, output_dir, degnorm_iter=args.iter,
                     nmf_iter=args.nmf_iter, downsample_rate=args.downsample_rate, minimax_coverage=args.minimax_coverage,
                     skip_baseline_selection=args.skip_baseline_selection, unique_alignment=not args.non_unique_alignments,
                     n_jobs=args.proc_per_node, inflate='device' if args.device_inflate else 'host',
                     frame='device' if args.device_frame else 'host', verify=verify,
                     pair='device' if getattr(args, 'device_pair', False) else 'host', pairing=getattr(args, 'pair_by', 'name'),
                     exclude_flags=getattr(args, 'exclude_flags', 0), require_flags=getattr(args, 'require_flags', 0),
                     min_mapq=getattr(args, 'min_mapq', 0), stranded=getattr(args, 'stranded', 'no'))
    logging.info('DegNorm pipeline complete! Exiting...')


def main(argv=None):
    args = validate_args(argparser().parse_args(argv))
    fmt = {'format': 'DegNorm (%(asctime)s) ---- %(message)s', 'datefmt': '%m/%d/%Y %I:%M:%S'}
    logging.basicConfig(level=logging.INFO, handlers=[logging.StreamHandler()], **fmt)
    device, verify = int(os.environ.get('LOCAL_RANK', 0)), getattr(args, 'verify_crc', False)
    # the missing index files first: a file that cannot be indexed stops the run before an output directory exists
    for k, bam_file in enumerate(args.create_bai_files or []):
        from .utils import create_index_file
        logging.info('creating index file for {0} -- {1} / {2}'.format(bam_file, k + 1, len(args.create_bai_files)))
        create_index_file(bam_file, device=device, verify=verify, fmt=args.index_format)
    output_dir = create_output_dir(args.output_dir)
    log_file = logging.FileHandler(os.path.join(output_dir, 'degnorm.log'))
    log_file.setFormatter(logging.Formatter(fmt['format'], fmt['datefmt']))
    logging.getLogger().addHandler(log_file)
    try:
        _run(args, output_dir, device, verify)
    finally:                                             # a later call in this process logs to its own file only
        logging.getLogger().removeHandler(log_file)
        log_file.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())

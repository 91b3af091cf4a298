"""
Host side of the BAM + GTF pipeline, no device: merge_read_counts and merge_overlap_gene_coverage on per-sample files
written from the reference's golden (tests/golden/pipeline.npz) against the reference's merged tables, and the command
line of `python -m degnorm_amd`: its validation rules, its output-directory rules and --help in a child process.
"""
import argparse
import os
import pickle
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from conftest import golden                                            # noqa: E402
from test_annotation_host import golden_frame                          # noqa: E402
from degnorm_amd import __main__ as cli                                # noqa: E402
from degnorm_amd.coverage_merge import merge_overlap_gene_coverage, merge_read_counts       # noqa: E402


def write_sample_files(z, data_dir, skip=()):
    """The per-sample read count and overlap coverage files the reference wrote when the golden was made."""
    samples, chroms = z['sample_ids'].tolist(), z['chroms'].tolist()
    for s in samples:
        os.makedirs(os.path.join(data_dir, s), exist_ok=True)
        for c in chroms:
            if ('counts', s, c) not in skip:
                pd.DataFrame({'gene': z['counts_{0}_genes'.format(c)], s: z['counts_{0}_{1}'.format(c, s)]}).to_csv(
                    os.path.join(data_dir, s, 'read_counts_{0}_{1}.csv'.format(s, c)), index=False)
            if ('ol', s, c) not in skip:
                off = np.r_[0, np.cumsum(z['ol_{0}_len'.format(c)])]
                flat = z['ol_{0}_{1}'.format(c, s)]
                with open(os.path.join(data_dir, s, 'overlap_coverage_{0}_{1}.pkl'.format(s, c)), 'wb') as f:
                    pickle.dump({g: flat[off[k]:off[k + 1]] for k, g in enumerate(z['ol_{0}_genes'.format(c)].tolist())}, f)
    return samples, chroms


def test_merge_read_counts_equals_reference(tmp_path):
    z = golden('pipeline')
    samples, chroms = write_sample_files(z, str(tmp_path))
    got = merge_read_counts(str(tmp_path), samples, chroms)
    expect = golden_frame(z, 'merged_counts', ['chr', 'gene'] + samples)
    pd.testing.assert_frame_equal(got, expect)
    assert got.columns.tolist() == ['chr', 'gene'] + samples and not got.index.is_unique     # the concatenated index, not reset
    os.remove(os.path.join(str(tmp_path), samples[1], 'read_counts_{0}_{1}.csv'.format(samples[1], chroms[1])))
    with pytest.raises(FileNotFoundError, match='read counts file .* not available!'):
        merge_read_counts(str(tmp_path), samples, chroms)


def test_merge_overlap_gene_coverage_equals_reference(tmp_path):
    z = golden('pipeline')
    samples, chroms = write_sample_files(z, str(tmp_path))
    for c in chroms:
        got = merge_overlap_gene_coverage(str(tmp_path), samples, c)
        genes, lens = z['merged_ol_{0}_genes'.format(c)].tolist(), z['merged_ol_{0}_len'.format(c)]
        off = np.r_[0, np.cumsum(lens * len(samples))]
        assert list(got) == genes and len(genes) > 0
        for k, g in enumerate(genes):
            assert got[g].dtype == np.float64 and got[g].shape == (len(samples), lens[k])
            np.testing.assert_array_equal(got[g].reshape(-1), z['merged_ol_{0}_flat'.format(c)][off[k]:off[k + 1]])
    os.remove(os.path.join(str(tmp_path), samples[2], 'overlap_coverage_{0}_{1}.pkl'.format(samples[2], chroms[0])))
    assert merge_overlap_gene_coverage(str(tmp_path), samples, chroms[0]) == {}


def _args(**kw):
    base = dict(bam_files=None, bai_files=None, bam_dir=None, warm_start_dir=None, genome_annotation=None, output_dir=None,
                downsample_rate=1, nmf_iter=100, iter=5, minimax_coverage=0, skip_baseline_selection=False,
                non_unique_alignments=False, proc_per_node=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_cli_validation(tmp_path):
    d = str(tmp_path)
    gtf = os.path.join(d, 'a.gtf')
    open(gtf, 'w').close()
    bams = [os.path.join(d, n) for n in ('s1.bam', 's2.bam')]
    for b in bams:
        open(b, 'w').close()
    with pytest.raises(ValueError, match='Must specify either --bam-files, --bam-dir, or --warm-start-dir'):
        cli.validate_args(_args())
    for bad in (dict(nmf_iter=0), dict(iter=0), dict(downsample_rate=0)):
        with pytest.raises(ValueError, match='must all be >= 1'):
            cli.validate_args(_args(bam_files=bams, genome_annotation=gtf, **bad))
    with pytest.raises(ValueError, match='gene annotation file must be specified'):
        cli.validate_args(_args(bam_files=bams))
    with pytest.raises(FileNotFoundError, match='Gene annotation file'):
        cli.validate_args(_args(bam_files=bams, genome_annotation=os.path.join(d, 'none.gtf')))
    with pytest.raises(ValueError, match='is not a .bam file'):
        cli.validate_args(_args(bam_files=[gtf, bams[0]], genome_annotation=gtf))
    with pytest.raises(FileNotFoundError, match='.bam file'):
        cli.validate_args(_args(bam_files=[bams[0], os.path.join(d, 'none.bam')], genome_annotation=gtf))
    with pytest.raises(FileNotFoundError, match='No .bai index file .*s1.bai'):                 # no samtools shell-out
        cli.validate_args(_args(bam_files=bams, genome_annotation=gtf))
    bais = [b[:-3] + 'bai' for b in bams]
    for b in bais:
        open(b, 'w').close()
    with pytest.raises(ValueError, match='Number of supplied .bai files'):
        cli.validate_args(_args(bam_files=bams, bai_files=bais[:1], genome_annotation=gtf))
    with pytest.raises(ValueError, match='is not a .bai file'):
        cli.validate_args(_args(bam_files=bams, bai_files=[bais[0], gtf], genome_annotation=gtf))
    with pytest.raises(ValueError, match='Fewer than 2 .bam files'):
        cli.validate_args(_args(bam_files=bams[:1], genome_annotation=gtf))
    with pytest.raises(ValueError, match='not uniquely named'):
        cli.validate_args(_args(bam_files=[bams[0], bams[0]], genome_annotation=gtf))
    with pytest.raises(ValueError, match='Do not specify both a --bam-dir'):
        cli.validate_args(_args(bam_dir=d, bam_files=bams, genome_annotation=gtf))
    with pytest.raises(NotADirectoryError, match='--bam-dir'):
        cli.validate_args(_args(bam_dir=os.path.join(d, 'nodir'), genome_annotation=gtf))
    with pytest.raises(NotADirectoryError, match='--warm-start-dir'):
        cli.validate_args(_args(warm_start_dir=os.path.join(d, 'nodir')))
    ok = cli.validate_args(_args(bam_files=bams, genome_annotation=gtf))
    assert ok.bam_files == bams and ok.bai_files == bais                                         # the .bai next to each .bam
    ok = cli.validate_args(_args(bam_dir=d, genome_annotation=gtf))
    assert ok.bam_files == bams and ok.bai_files == bais
    ok = cli.validate_args(_args(warm_start_dir=d, bam_files=bams, genome_annotation=gtf))
    assert ok.bam_files is None and ok.genome_annotation is None
    one = tmp_path / 'one'
    one.mkdir()
    open(str(one / 'x.bam'), 'w').close()
    with pytest.raises(ValueError, match='Only found 1 .bam'):
        cli.validate_args(_args(bam_dir=str(one), genome_annotation=gtf))


def test_cli_flags_are_the_references():
    ns = cli.argparser().parse_args(['--bam-files', 'a.bam', 'b.bam', '--bai-files', 'a.bai', 'b.bai', '-g', 'x.gtf', '-o', 'out', '-d', '4',
                                     '--nmf-iter', '20', '--iter', '3', '--minimax-coverage', '7', '-s', '--non-unique-alignments', '-p', '2'])
    assert (ns.bam_files, ns.bai_files, ns.genome_annotation, ns.output_dir) == (['a.bam', 'b.bam'], ['a.bai', 'b.bai'], 'x.gtf', 'out')
    assert (ns.downsample_rate, ns.nmf_iter, ns.iter, ns.minimax_coverage, ns.proc_per_node) == (4, 20, 3, 7, 2)
    assert ns.skip_baseline_selection and ns.non_unique_alignments
    ns = cli.argparser().parse_args(['--bam-dir', 'd', '-w', 'prev'])
    assert (ns.bam_dir, ns.warm_start_dir, ns.downsample_rate, ns.nmf_iter, ns.iter, ns.minimax_coverage, ns.proc_per_node) == \
        ('d', 'prev', 1, 100, 5, 0, 1)


def test_output_directory_rules(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    made = cli.create_output_dir(None)                                   # none given: ./degnorm_<date>_<time>
    assert os.path.dirname(made) == os.getcwd() and os.path.basename(made).startswith('degnorm_') and os.path.isdir(made)
    inside = cli.create_output_dir(made)                                 # an existing directory: a dated one inside it
    assert os.path.dirname(inside) == made and os.path.basename(inside).startswith('degnorm_') and os.path.isdir(inside)
    bare = cli.create_output_dir('fresh')                                # a bare new name: in the working directory
    assert bare == os.path.join(os.getcwd(), 'fresh') and os.path.isdir(bare)
    deep = cli.create_output_dir(os.path.join(str(tmp_path), 'a', 'b'))  # a new path: itself
    assert deep == os.path.join(str(tmp_path), 'a', 'b') and os.path.isdir(deep)


def test_help_exits_zero_in_a_child_process():
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd', '--help'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    for flag in ('--bam-files', '--bai-files', '--bam-dir', '--warm-start-dir', '--genome-annotation', '--output-dir',
                 '--downsample-rate', '--nmf-iter', '--iter', '--minimax-coverage', '--skip-baseline-selection',
                 '--non-unique-alignments', '--proc-per-node'):
        assert flag in r.stdout
    for missing in ('--plot-genes', 'report', '.bai', 'MPI'):
        assert missing in r.stdout

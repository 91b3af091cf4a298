"""
GPU tests of the coverage-text formatter (dn_cov_text, csrc/dn_text.hip; degnorm_amd.data_access): the device against the host
build byte for byte, offsets and flags included, on every case of tests/_text_cases.py (tests/test_text_host.py holds the host
build to Python's '%.5f' and to pandas) -- among them 256 x 70, whose wavefronts build their runs in many LDS chunks, and the
mixed batch, cut into three batches as well; get_coverage_data with formatter='device' against the files of the real
reference (tests/golden/data_access.npz), against the pandas formatter on a directory with a NaN gene and on one with a
quoted sample id; and `python -m degnorm_amd.data_access` on the directory run_pipeline writes for the pipeline golden's
three samples.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _bam_fixtures as bf                                     # noqa: E402
import _data_access_fixtures as daf                            # noqa: E402
import _gtf_fixtures as gf                                     # noqa: E402
import _text_cases as tc                                       # noqa: E402
from conftest import golden, GOLDEN                            # noqa: E402
from degnorm_amd import _lib, data_access as da                # noqa: E402
from degnorm_amd.pipeline import run_pipeline                  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_device_text_equals_host_text(name):
    p, mats, flagged = tc.CASES[name]
    with da.cov_text(mats, host=True) as h, da.cov_text(mats, device=0) as d:
        assert set(np.flatnonzero(d.flag).tolist()) == flagged
        assert d.flag.tolist() == h.flag.tolist() and d.off.tolist() == h.off.tolist() and d.size == h.size
        assert bytes(d.view) == bytes(h.view)
        assert d.size == 0 or d.ms[3] > 0                        # the emit kernel ran


def test_three_device_batches_equal_one():
    p, mats, _ = tc.CASES['mixed']
    budget = 8 * sum(m.size for m in mats) // 3
    one, one_flag, n_one = da.cov_text_pieces(mats, device=0)
    three, three_flag, n_three = da.cov_text_pieces(mats, device=0, batch_bytes=budget)
    host = da.cov_text_pieces(mats, host=True)[0]
    assert (n_one, n_three) == (1, 3)
    assert three == one == host and three_flag.tolist() == one_flag.tolist() == [0] * len(mats)


def test_unknown_device_is_refused():
    with pytest.raises(ValueError, match='dn_cov_text: device index out of range'):
        da.cov_text([np.ones((2, 3))], device=_lib.device_count())
    with pytest.raises(ValueError, match='dn_cov_text: device index out of range'):
        da.cov_text([np.ones((2, 3))], device=-1)


def test_device_formatter_writes_the_reference_files(tmp_path):
    z = golden('data_access')
    files = {p: z['file_{0}'.format(k)].tobytes() for k, p in enumerate(z['paths'].tolist())}
    src, save = daf.write_reference_dir(str(tmp_path / 'out')), str(tmp_path / 'saved')
    stats = {}
    out = da.get_coverage_data(daf.REFERENCE_GENES, src, save_dir=save, device=0, n_jobs=2, stats=stats)      # 'device' is the default
    assert daf.tree(save) == files
    assert list(out) == z['genes'].tolist() and list(out['GENE_1']['raw'].columns) == z['columns'].tolist()
    assert stats['batches'] == 1 and stats['flagged_files'] == 0 and stats['emit_ms'] > 0
    assert stats['text_bytes'] == sum(len(b) - len(b'sample_1 sample_2\n') for b in files.values())
    # one file a batch
    save2 = str(tmp_path / 'saved2')
    da.get_coverage_data('all', src, save_dir=save2, device=0, batch_bytes=1, stats=stats)
    assert daf.tree(save2) == files and stats['batches'] == 4


@pytest.mark.parametrize('which', ['nan', 'hard'])
def test_device_formatter_equals_pandas_formatter(which, tmp_path):
    src = (daf.write_nan_dir if which == 'nan' else daf.write_hard_dir)(str(tmp_path / 'out'))
    dev, ref = str(tmp_path / 'device'), str(tmp_path / 'pandas')
    stats = {}
    da.get_coverage_data('all', src, save_dir=dev, device=0, stats=stats)
    da.get_coverage_data('all', src, save_dir=ref, formatter='pandas')
    got, want = daf.tree(dev), daf.tree(ref)
    assert sorted(got) == sorted(want) and len(want) == (6 if which == 'nan' else 8)
    assert got == want
    assert stats['flagged_files'] == (2 if which == 'nan' else 0)        # B2's raw (an infinity) and estimate (NaNs)


def test_command_line_on_a_pipeline_directory(tmp_path):
    z = golden('pipeline')
    bams = []
    for k, s in enumerate(gf.PIPELINE_SAMPLES):
        path = str(tmp_path / (s + '.bam'))
        bf.write_bam(path, gf.PIPELINE_REFS, gf.pipeline_bam_rows(k), straddle=(k == 1))
        bams.append(path)
    out = str(tmp_path / 'out')
    os.makedirs(out)
    model, estimates, cov, *_ = run_pipeline(bams, [b + '.bai' for b in bams], os.path.join(GOLDEN, 'pipeline.gtf'), out, degnorm_iter=3,
                                             nmf_iter=50, minimax_coverage=int(z['case_a_minimax']), verbose=False)
    genes = list(cov)[:3]
    dev, ref = str(tmp_path / 'device'), str(tmp_path / 'pandas')
    r = subprocess.run([sys.executable, '-m', 'degnorm_amd.data_access', '-d', out, '-g'] + [g.lower() for g in genes] + ['-o', dev, '--device', '0'],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert '3 genes' in r.stdout
    da.get_coverage_data(genes, out, save_dir=ref, formatter='pandas')
    got, want = daf.tree(dev), daf.tree(ref)
    assert len(want) == 6 and {os.path.basename(p).split('_')[0] for p in want} == {g.upper() for g in genes}
    assert got == want
    header = (' '.join(gf.PIPELINE_SAMPLES) + '\n').encode()
    assert all(b.startswith(header) for b in got.values())

"""
bench.py on the device at a small size, once plain and once with --full: a plain run prints the headline line and nothing that
needs runs of its own; --full adds the post-clock checks, the CPU baseline, the end-to-end timing and the stream-read ceiling.
Both runs time the same steps, so what they dump is the same.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
SMALL = ['--gpus', '1', '--genes', '400', '--steps', '1', '--warmup', '1', '--parity-genes', '16']

pytestmark = pytest.mark.gpu


def _bench(*argv):
    r = subprocess.run([sys.executable, BENCH] + SMALL + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs(tmp_path):
    plain = _bench('--dump-outputs', str(tmp_path / 'plain'))
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in plain
    assert plain['value'] > 0 and plain['ms_per_step'] > 0 and plain['unit'] == 'genes/sec' and plain['dtype'] == 'f64'
    assert plain['full'] is False and plain['parity'] is None and plain['cpu_baseline'] is None
    assert 'end_to_end' not in plain and 'also' not in plain
    assert plain['roofline']['stream_read_ceiling_gbps'] is None

    full = _bench('--full', '--cpu-sample', '24', '--cpu-single', '4', '--dump-outputs', str(tmp_path / 'full'))
    assert full['full'] is True and full['metric'] == plain['metric']
    assert full['parity']['ok'] and full['parity']['genes_checked'] > 0 and full['parity']['chain']['genes'] == 24
    assert full['cpu_baseline']['value'] > 0 and full['end_to_end']['genes_per_s'] > 0
    assert full['roofline']['stream_read_ceiling_gbps'] > 0

    names = sorted(os.listdir(str(tmp_path / 'plain')))
    assert names == sorted(os.listdir(str(tmp_path / 'full'))) and 'rho.npy' in names
    for n in names:
        np.testing.assert_array_equal(np.load(str(tmp_path / 'plain' / n)), np.load(str(tmp_path / 'full' / n)))

"""bench.py's plain run and --dump-outputs at small size: a plain run times
--steps steps and leaves the --full legs out of its line, and the outputs it
dumps (float32 / float64 .npy, under 64 MB) are the same from run to run with
the same arguments, whatever the number of steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

PAIRS = 20000      # 40000 records: more than the 32768 the dump samples


def _bench(args):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py')] + args, env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp('dump')
    out = []
    for k, steps in enumerate((1, 3)):
        d = str(base / ('run%d' % k))
        line = _bench(['--gpus', '1', '--pairs', str(PAIRS), '--steps', str(steps), '--warmup', '1',
                       '--dump-outputs', d])
        out.append((line, d))
    return out


def test_plain_line(runs):
    for (line, _), steps in zip(runs, (1, 3)):
        assert line['steps'] == steps and line['warmup'] == 1 and line['n_gpus'] == 1
        assert line['ms_per_step'] > 0 and line['value'] > 0
        assert line['unit'] == 'reads/s' and line['higher_is_better'] is True and line['dtype'] == 'int32'
        # value is reads over the timed steps: 2 * pairs * steps / (steps * ms_per_step)
        assert line['value'] == pytest.approx(2 * PAIRS / (line['ms_per_step'] / 1e3), rel=1e-3)
        for leg in ('cpu_baseline', 'parity', 'end_to_end', 'end_to_end_single_member'):
            assert line[leg] is None, leg
        # one launch of the dominant kernel per mapping pass per timed step
        assert line['roofline']['launches'] % steps == 0


def test_dump_is_reproducible_and_bounded(runs):
    (line, a), (_, b) = runs
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    assert names == sorted(f for f in os.listdir(b) if f.endswith('.npy'))
    assert {'conseq_0.npy', 'mapped_counts.npy', 'unmapped.npy', 'records.npy',
            'records_index.npy'} <= set(names)
    total = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64), f
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f
        total += x.nbytes
    assert total <= 64 * 2 ** 20
    # the dump says what the line says
    conseq = np.load(os.path.join(a, 'conseq_0.npy'))
    with open(os.path.join(a, 'conseq_names.txt')) as f:
        cnames = f.read().split()
    assert cnames == list(line['result']['conseqs'])
    assert len(conseq) == line['result']['conseqs'][cnames[0]]
    assert conseq.min() >= 32 and conseq.max() < 127      # character codes
    counts = np.load(os.path.join(a, 'mapped_counts.npy'))
    assert counts.tolist() == [line['result']['mapped_lines'][n] for n in cnames]
    # a sample of whole blocks of records, each with its read index
    idx = np.load(os.path.join(a, 'records_index.npy'))
    rec = np.load(os.path.join(a, 'records.npy'))
    assert len(idx) == len(rec) == 32768 and len(np.unique(idx)) == len(idx)
    assert idx.min() >= 0 and idx.max() < 2 * PAIRS
    assert (rec == np.round(rec)).all()

"""amino_detail.csv from a sharded aln2counts: two ranks on the test box's one
GPU (gloo) each count the codon classes of the rows in their share of
aligned.csv (k_a2c_detail after mh_a2c_part_count), the [codon][3] tables are
added up over the ranks (micall_amd.aln2counts._job_detail) and rank 0
writes.  Rank 0's file must equal the single-process file, which
tests/test_gpu_amino_detail.py holds to the oracle; also when only rank 0
was given amino_detail_csv (every rank enters the sum all the same)."""
import gzip
import io
import json
import os
import socket
import subprocess
import sys

import pytest

import clip_oracle
import ins_oracle
from micall_amd import aln2counts as a2c

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
WORKER = os.path.join(HERE, 'gpu_amino_detail_worker.py')
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'amino_detail')
WORLD = 2


def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _gz(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.csv.gz'), 'rt') as f:
        return f.read()


def _single(texts):
    """The five outputs of a single-process call on the case's texts."""
    outs = {k: io.StringIO() for k in OUTS}
    a2c.aln2counts(io.StringIO(texts['aligned']), outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'],
                   clipping_csv=io.StringIO(texts['clipping']) if 'clipping' in texts else None,
                   conseq_ins_csv=io.StringIO(texts['conseq_ins']) if 'conseq_ins' in texts else None,
                   amino_detail_csv=outs['amino_detail'])
    return {k: v.getvalue() for k, v in outs.items()}


@pytest.mark.timeout(300)
def test_two_ranks_write_the_single_process_file(tmp_path):
    remap = _gz('syn_pol_indel', 'remap')
    indel = dict(aligned=_gz('syn_pol_indel', 'aligned'), clipping=clip_oracle.clipping(remap)[0],
                 conseq_ins=ins_oracle.conseq_ins(remap))
    cases = {'both_syn_pol_indel': indel, 'rank0_syn_pol_indel': indel,
             'both_c1_example': dict(aligned=_gz('c1_example', 'aligned'))}
    root = tmp_path / 'cases'
    for name, texts in cases.items():
        os.makedirs(root / name)
        for k, text in texts.items():
            (root / name / (k + '.csv')).write_text(text)
    want = {name: _single(texts) for name, texts in cases.items()}
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE=str(WORLD),
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, WORKER, '--cases', str(root)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(WORLD)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0] * WORLD, codes
    stats = [json.load(open(root / ('rank%d.json' % r))) for r in range(WORLD)]
    for name in cases:
        assert [s[name].get('mode') for s in stats] == ['sharded'] * WORLD, name
        rows = [s[name]['rows'] for s in stats]
        assert max(rows) < sum(rows), (name, rows)
        for k in OUTS:
            with open(root / name / (k + '.csv'), newline='') as f:
                assert f.read() == want[name][k], (name, k)
        detail = want[name]['amino_detail'].splitlines()
        assert len(detail) > 100
        assert sum(1 for line in detail[1:] if int(line.split(',')[27]) > 0) > 300    # partial

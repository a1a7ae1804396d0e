"""sam2aln at several q-cutoffs in one device pass (mh_sam2aln_csv_q,
mh_sam2aln_file_q, micall_amd.sam2aln with q_cutoffs): byte-equal to the
reference's own outputs with its SAM2ALN_Q_CUTOFFS list patched
(tests/golden/sam2aln_qcuts.json) and, on larger synthetic remap.csv texts,
to the oracle restatement (oracle/og_sam2aln.py, pinned on the same goldens by
tests/test_oracle_sam2aln_qcuts.py).  Reference: sam2aln.py:391-402 (the loop
over the cutoffs), :446-452 and :466-467 (the group order)."""
import csv
import ctypes
import io
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import og_aln2counts
import og_sam2aln
import s2a_qcuts_cases as qc
from micall_amd import _native, projects, synth
from micall_amd import aln2counts as a2c
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'gpu_s2a_qcuts_worker.py')
LISTS = ([0, 10, 15], [15, 10, 0])


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _device(ctx, text, cuts):
    ctx.sam2aln_csv(text, q_cutoffs=cuts)
    return ctx.sam2aln_output('aligned'), ctx.sam2aln_output('insert'), ctx.sam2aln_output('failed')


def _oracle(text, cuts):
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = list(cuts)
    try:
        return og_sam2aln.sam2aln(text)
    finally:
        og_sam2aln.Q_CUTOFFS = saved


def _mapped_remap_csv(ctx, n_pairs, seed):
    """remap.csv text from the GPU mapper (--local vs HIV pol) on synthetic
    reads with indels, Ns and low-quality stretches, as
    tests/test_gpu_sam2aln.py builds it."""
    pol = projects.load_default().seed_sequences()['HIV1B-pol-seed']
    pairs = synth.make_pairs(n_pairs, genomes={'HIV1B-pol-seed': pol}, genome_seed=seed,
                             read_seed=seed + 1, indel_rate=0.01, err_rate=0.02)
    names, seqs, quals = synth.interleave(pairs)
    rng = np.random.default_rng(seed)
    quals = [q if rng.random() > 0.05 else '#' * len(q) for q in quals]
    ctx.index_build(['HIV1B-pol-seed'], [pol], 20)
    names = [n[1:].split()[0] for n in names]      # bowtie2's QNAME: mates share it
    ctx.reads_load(seqs, quals, True, names=names)
    ctx.map(_native.params(_native.LOCAL))
    return qc.HEAD + ctx.format_rows(1, 0, len(seqs))


def _requalify(rows, seed):
    """Both mates of a random 5 % of the qnames get quality '-' (Q12)
    throughout, another 5 % '#' (Q2): pairs that pass at some cutoffs only,
    and pairs that pass at 0 alone or not at all."""
    names = sorted({r[0] for r in rows})
    rng = np.random.default_rng(seed)
    draw = rng.random(len(names))
    fill = {n: '-' for n, d in zip(names, draw) if d < 0.05}
    fill.update({n: '#' for n, d in zip(names, draw) if 0.05 <= d < 0.10})
    return [r[:10] + [fill[r[0]] * len(r[10])] if r[0] in fill else r for r in rows]


def _csv_text(rows):
    out = io.StringIO()
    csv.writer(out, lineterminator='\n').writerows(rows)
    return out.getvalue()


@pytest.fixture(scope='module')
def big_text(ctx):
    """3 000 mapped pairs, the first 1 200 rows again under new qnames
    (counts > 1), 10 % of the pairs at a flat low quality."""
    rows = list(csv.reader(io.StringIO(_mapped_remap_csv(ctx, 3000, 41))))
    body = rows[1:] + [[r[0] + 'x'] + r[1:] for r in rows[1:1201]]
    return _csv_text([rows[0]] + _requalify(body, 43))


@pytest.fixture(scope='module')
def small_text(ctx):
    """300 mapped pairs, 10 % of them at a flat low quality."""
    rows = list(csv.reader(io.StringIO(_mapped_remap_csv(ctx, 300, 47))))
    return _csv_text([rows[0]] + _requalify(rows[1:], 49))


@pytest.fixture(scope='module')
def small_want(small_text):
    return _oracle(small_text, [0, 10, 15])


# ---- the reference's own outputs -------------------------------------------
@pytest.mark.parametrize('k', range(len(qc.CASES)), ids=qc.case_id)
def test_matches_reference_at_every_cutoff_list(ctx, k):
    """The library is given the list as the drop-in hands it over: repeats
    dropped ([15, 15] is [15], the reference's mseqs[qcut] being a dict)."""
    case = qc.CASES[k]
    got = _device(ctx, qc.remap_text(case), s2a._cutoff_list(case['q_cutoffs']))
    for name, text in zip(('aligned', 'insert', 'failed'), got):
        qc.assert_equals_golden(text, case[name], (case['name'], case['q_cutoffs'], name))


def test_groups_come_in_first_success_order(ctx):
    """p1 fails at 15 and passes at 10 and 0, p2 passes everywhere, p3
    nowhere: the groups are 10, 0, 15 and failed.csv has one row per pair."""
    al, ins, fa = _device(ctx, qc.tiny_text(), [15, 10, 0])
    assert al == ('refname,qcut,rank,count,offset,seq\n'
                  'R,10,0,2,0,ACGTACGT\n'
                  'R,0,0,2,0,ACGTACGT\n'
                  'R,15,0,1,0,ACGTACGT\n')
    assert fa == 'qname,cause\np1,manyNs\np3,manyNs\n'
    assert ins == 'qname,fwd_rev,refname,pos,insert,qual\n'
    # pairs, merged on the device, rows of aligned.csv, rows of failed.csv
    assert list(ctx.sam2aln_stats()) == [3, 3, 3, 2]


def test_gap_held_by_a_read_moves_the_offset_between_cutoffs(ctx):
    """A '-' in the seq column comes with the read's own quality: at cutoff 0
    it beats the mate's Q0 base (a gap: offset 2), at 30 it is censored (N:
    offset 0).  Offsets and stripped lengths are per cutoff."""
    text = (qc.HEAD + 'g1,99,R,1,44,8M,=,1,8,--GTACGT,55IIIIII\n'
                      'g1,147,R,1,44,8M,=,1,8,ACGTACGT,!!IIIIII\n')
    want = _oracle(text, [0, 30])
    assert want[0] == ('refname,qcut,rank,count,offset,seq\n'
                       'R,0,0,1,2,GTACGT\n'
                       'R,30,0,1,0,NNGTACGT\n')
    assert _device(ctx, text, [0, 30]) == want


# ---- against the oracle ----------------------------------------------------
def _group_counts(aligned):
    tot = {}
    for row in csv.DictReader(io.StringIO(aligned)):
        tot[int(row['qcut'])] = tot.get(int(row['qcut']), 0) + int(row['count'])
    return tot


@pytest.mark.parametrize('cuts', LISTS, ids=lambda c: '_'.join(map(str, c)))
def test_vs_oracle_synthetic(ctx, big_text, cuts):
    want = _oracle(big_text, cuts)
    # the input does what it is meant to (judged on the oracle's output)
    tot = _group_counts(want[0])
    assert tot[15] + 50 <= tot[10] and tot[10] + 50 <= tot[0], tot
    failing = [line.split(',')[0] for line in want[2].splitlines()[1:]]
    assert len(failing) > 100 and len(set(failing)) == len(failing)
    got = _device(ctx, big_text, cuts)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    st = ctx.sam2aln_stats()
    assert st[0] == 3600 and st[2] == want[0].count('\n') - 1 and st[3] == len(failing), st


def test_drop_in_on_handles(small_text, small_want):
    al, ins, fa = io.StringIO(), io.StringIO(), io.StringIO()
    s2a.sam2aln(io.StringIO(small_text), al, ins, fa, q_cutoffs=[0, 10, 15])
    assert (al.getvalue(), ins.getvalue(), fa.getvalue()) == small_want


def test_drop_in_on_files(tmp_path, small_text, small_want):
    """Real files: remap.csv mmap'd by the library (mh_sam2aln_file_q), the
    outputs written by it at the handles' positions."""
    rp = tmp_path / 'remap.csv'
    rp.write_text(small_text)
    outs = {k: tmp_path / (k + '.csv') for k in ('aligned', 'insert', 'failed')}
    with open(rp) as remap, open(outs['aligned'], 'w') as al, open(outs['insert'], 'w') as ins, \
            open(outs['failed'], 'w') as fa:
        s2a.sam2aln(remap, al, ins, fa, q_cutoffs=[0, 10, 15])
    assert tuple(outs[k].read_text() for k in ('aligned', 'insert', 'failed')) == small_want


def test_drop_in_reads_the_module_constant(monkeypatch, small_text, small_want):
    """Where the reference's users set the list."""
    monkeypatch.setattr(s2a, 'SAM2ALN_Q_CUTOFFS', [0, 10, 10, 15])
    al, ins, fa = io.StringIO(), io.StringIO(), io.StringIO()
    s2a.sam2aln(io.StringIO(small_text), al, ins, fa)
    assert (al.getvalue(), ins.getvalue(), fa.getvalue()) == small_want


def test_chain_into_aln2counts(small_want):
    """The multi-cutoff aligned.csv through micall_amd.aln2counts: rows for
    every cutoff, byte-equal to the oracle's aln2counts on the same text."""
    outs_names = ('nuc', 'amino', 'coord_ins', 'conseq', 'failed', 'coverage')
    outs = {k: io.StringIO() for k in outs_names}
    a2c.aln2counts(io.StringIO(small_want[0]), outs['nuc'], outs['amino'], outs['coord_ins'],
                   outs['conseq'], failed_align_csv=outs['failed'],
                   coverage_summary_csv=outs['coverage'])
    want = og_aln2counts.aln2counts(small_want[0], og_aln2counts.default_projects())
    for k in outs_names:
        assert outs[k].getvalue() == want[k], k
    cuts = {row['q-cutoff'] for row in csv.DictReader(io.StringIO(outs['nuc'].getvalue()))
            if row['seed'] == 'HIV1B-pol-seed'}
    assert cuts == {'0', '10', '15'}


# ---- the C entry points ----------------------------------------------------
def _call_q(ctx, text, cuts, n_cut=None):
    data = text.encode()
    arr = np.asarray(cuts, dtype=np.int32)
    n = ctypes.c_int64()
    return _native.lib().mh_sam2aln_csv_q(ctx.h, data, len(data), len(arr) if n_cut is None else n_cut,
                                          arr.ctypes.data_as(ctypes.c_void_p), 0.5, ctypes.byref(n))


@pytest.mark.parametrize('cuts,n_cut', [([15], 0), (list(range(9)), 9), ([15, -1], None),
                                        ([94], None), ([15, 10, 15], None)])
def test_bad_cutoff_arguments_are_refused(ctx, tmp_path, cuts, n_cut):
    case = qc.E2E_JSON[9]
    assert _call_q(ctx, case['remap_csv'], cuts, n_cut) == -3
    assert 'cutoff' in _native.last_error()
    rp = tmp_path / 'remap.csv'
    rp.write_text(case['remap_csv'])
    with open(rp) as f:
        with pytest.raises(_native.NativeError, match='cutoff'):
            ctx.sam2aln_file(f.fileno(), q_cutoffs=cuts if n_cut is None else cuts[:n_cut])
    # the context is as good as before
    ctx.sam2aln_csv(case['remap_csv'])
    assert ctx.sam2aln_output('aligned') == case['aligned']
    assert ctx.sam2aln_output('failed') == case['failed']


@pytest.mark.parametrize('k', [8, 9])
def test_one_cutoff_through_the_list_call_is_the_single_call(ctx, k):
    text = qc.E2E_JSON[k]['remap_csv']
    ctx.sam2aln_csv(text)
    want = tuple(ctx.sam2aln_output(w) for w in ('aligned', 'insert', 'failed'))
    stats = list(ctx.sam2aln_stats())
    assert _device(ctx, text, [15]) == want
    assert list(ctx.sam2aln_stats()) == stats
    assert want[0] == qc.E2E_JSON[k]['aligned']


# ---- a sharded job ---------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_sharded_job_takes_the_rank0_route(tmp_path, small_text):
    """world = 2 (gloo, one GPU): with three cutoffs no rank enters the split;
    rank 0 computes and writes, byte-equal to the oracle."""
    cuts = [15, 10, 0]
    rows = small_text.splitlines(keepends=True)
    text = qc.tiny_text() + ''.join(rows[1:401])      # the tiny example plus 200 synthetic pairs
    d = tmp_path / 'case'
    d.mkdir()
    (d / 'remap.csv').write_text(text)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, WORKER, '--case', str(d), '--qcuts', '15,10,0'],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=280) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    want = _oracle(text, cuts)
    for name, w in zip(('aligned', 'insert', 'failed'), want):
        assert (d / (name + '.csv')).read_text() == w, name
    for r in range(2):
        stats = json.load(open(str(d / ('rank%d.json' % r))))
        assert stats.get('mode') != 'sharded', (r, stats)

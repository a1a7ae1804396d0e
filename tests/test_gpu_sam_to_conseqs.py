"""remap.sam_to_conseqs / build_conseqs, their debug reports and remap()'s
debug files on the GPU (reference: micall/core/remap.py:141-370, 560-571,
758-760).

  * the public function on every case of pileup_golden.json (consensuses with
    their key order, distance reports) and debug_reports.json (the
    reference's report strings);
  * k_pileup's watching instances: source 0 (the mapper's records) against
    source 1 (the same alignments as SAM text) against the Python
    restatement of debug_report_cases.watched, counts and first units, on
    more than one block, and again through the event buffer's grow-and-retry;
  * the refusals;
  * remap(debug_file_prefix=...) byte-equal to the reference's files, at one
    rank and at two, and the loop they close: pass n's SAM file through
    sam_to_conseqs is pass n + 1's FASTA;
  * the chain remap() -> sam_to_conseqs() -> sam2aln() -> aln2counts() keeps
    its resident shortcuts.
"""
import gzip
import io
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import debug_report_cases as drc
import oracle
import test_gpu_parity as par
from micall_amd import _native, projects, session
from micall_amd import aln2counts as a2c
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a
from micall_amd.pipeline import CONSENSUS_Q_CUTOFF, Shard

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILE_CASES = ('micro_2070A-PR', 'micro_2090A-HCV', 'syn_maxremaps', 'syn_unpaired300')
SEEDS = projects.load_default().seed_sequences()
GAG = SEEDS['HIV1B-gag-seed']


def _cases(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)['cases']


# ---- the public function against the reference's answers ---------------------
def test_sam_to_conseqs_on_every_pileup_golden_case(golden_dir):
    cases = _cases(golden_dir, 'pileup_golden.json')
    assert len(cases) > 30
    filtered = 0
    for c in cases:
        report = None if c['distance_report'] is None else {}
        got = rm.sam_to_conseqs(io.StringIO(c['sam']), c['quality_cutoff'], seeds=c['seeds'],
                                is_filtered=c['is_filtered'], filter_coverage=c['filter_coverage'],
                                distance_report=report)
        assert list(got.items()) == list(c['conseqs'].items()), c['sam'][:300]
        assert report == c['distance_report']
        filtered += bool(c['distance_report'])
    assert filtered > 0                   # the distance filter ran


def test_debug_reports_equal_the_reference_strings(golden_dir):
    report_cases = drc.golden_cases(os.path.join(golden_dir, 'debug_reports.json'))
    for c in report_cases:
        reports = {tuple(k): None for k in c['keys']}
        rm.sam_to_conseqs(io.StringIO(c['sam']), c['quality_cutoff'], debug_reports=reports)
        assert list(reports) == [tuple(k) for k in c['keys']]
        assert [reports[tuple(k)] for k in c['keys']] == c['reports'], c['name']
    # an empty dict asks for nothing; a key that can never match reports ''
    c = report_cases[0]
    empty = {}
    rm.sam_to_conseqs(io.StringIO(c['sam']), debug_reports=empty)
    assert empty == {}
    odd = {('nowhere', 2): None, ('test', 0): None, ('test', 2): None, ('test', 999999): None}
    rm.sam_to_conseqs(io.StringIO(c['sam']), debug_reports=odd)
    assert odd == {('nowhere', 2): '', ('test', 0): '', ('test', 2): c['reports'][0],
                   ('test', 999999): ''}
    # no rows at all: no consensus, empty reports
    assert rm.sam_to_conseqs(io.StringIO('')) == {}
    none = {('test', 2): None}
    assert rm.sam_to_conseqs(io.StringIO('@SQ\tSN:test\n'), debug_reports=none, seeds={'test': 'ACGT'}) == {}
    assert none == {('test', 2): ''}


def test_build_conseqs_reads_a_file(golden_dir, tmp_path):
    c = next(c for c in _cases(golden_dir, 'pileup_golden.json')
             if c['quality_cutoff'] == CONSENSUS_Q_CUTOFF and c['seeds'] and not c['is_filtered'])
    path = tmp_path / 'x.sam'
    path.write_text(c['sam'])
    assert rm.build_conseqs(str(path), seeds=c['seeds']) == c['conseqs']


# ---- the watching instances: source 0, source 1, the restatement -------------
REFNAMES = ['HIV1B-pol-seed', 'HIV1B-gag-seed']
REFSEQS = [par.POL, GAG]


@pytest.fixture(scope='module')
def mapped():
    """2000 synthetic pairs on two references, their SAM lines and 64 keys,
    with the restatement's histogram (computed once)."""
    names, seqs, quals = par._reads(2000, 23, genomes=dict(zip(REFNAMES, REFSEQS)), indel_rate=0.01)
    keys = [(r, 40 + 40 * k) for r in (0, 1) for k in range(31)] + [(0, 1), (1, len(GAG) + 5000)]
    assert len(keys) == 64
    return dict(names=names, seqs=seqs, quals=quals, keys=keys)


def _both_sources(ctx, m, q=CONSENSUS_Q_CUTOFF):
    gpu = par._gpu_alns(ctx, REFNAMES, REFSEQS, oracle.LOCAL, m['seqs'], m['quals'], True)
    lens = [len(s) for s in REFSEQS]
    ctx.pileup_watch(m['keys'])
    try:
        ctx.pileup(0, q, lens)
        info0 = _native.pileup_info(ctx.h, 2)
        got0 = ctx.pileup_watch_fetch()
        sam = ''.join(par._sam_lines(gpu, m['names'], m['seqs'], m['quals'], REFNAMES, True))
        rows = ctx.rows_load_sam(sam)
        assert rows['names'] == REFNAMES
        ctx.pileup(1, q, lens)
        info1 = _native.pileup_info(ctx.h, 2)
        got1 = ctx.pileup_watch_fetch()
    finally:
        ctx.pileup_watch([])
    if 'want' not in m:
        want = drc.watched(sam, q, [(REFNAMES[r], p) for r, p in m['keys']])
        # matchmaker's unit -> pair number (a pair of two '*' rows is no unit)
        _n, units = oracle.matchmaker(sam.splitlines(True))
        qnames = [oracle.qname_of(n, True) for n in m['names'][::2]]
        pair_of = {name: k for k, name in enumerate(qnames)}
        to_pair = np.array([pair_of[u[0][0]] for u in units] + [0], dtype=np.int64)
        first0 = np.where(want[1] == drc.NEVER, drc.NEVER, to_pair[np.minimum(want[1], len(units))])
        m['want'] = (want[0], want[1], first0)
    return got0, got1, info0, info1


def _assert_agree(m, got0, got1):
    counts, first1, first0 = m['want']
    assert counts.sum() > 5000 and (counts.reshape(64, -1).sum(axis=1) > 0).sum() >= 55
    assert not counts[-1].any() and not got0[0][-1].any()       # the key past the counters
    assert np.array_equal(got1[0], counts) and np.array_equal(got1[1], first1)
    assert np.array_equal(got0[0], counts) and np.array_equal(got0[1], first0)


def test_watch_source0_source1_and_restatement_agree(mapped):
    ctx = _native.Context(0)
    try:
        got0, got1, info0, info1 = _both_sources(ctx, mapped)
        assert info0['blocks'] > 1 and info1['blocks'] > 1 and info0['n_units'] == 2000
        _assert_agree(mapped, got0, got1)
        assert ctx.retry_counts()['pileup_events'] == 0
        # the same pileups unwatched count the same consensus input
        ctx.pileup(1, CONSENSUS_Q_CUTOFF, [len(s) for s in REFSEQS])
        plain = ctx.pileup_fetch()
        ctx.pileup_watch(mapped['keys'])
        ctx.pileup(1, CONSENSUS_Q_CUTOFF, [len(s) for s in REFSEQS])
        ctx.pileup_watch([])
        seen = ctx.pileup_fetch()
        for k in ('dense', 'nflag', 'dflag', 'read_counts', 'first_unit', 'max_pos'):
            assert np.array_equal(plain[k], seen[k]), k
        assert plain['events'] == seen['events']
    finally:
        ctx.close()


def test_watch_counts_once_through_the_event_retry(mapped):
    """The event buffer starts tiny: run_pileup grows it and launches again;
    the histogram is zeroed before every attempt, so it is unchanged."""
    ctx = _native.Context(0)
    try:
        ctx.test_set_capacities(pileup_events=3, pileup_event_bytes=8)
        got0, got1, _i0, _i1 = _both_sources(ctx, mapped)
        assert ctx.retry_counts()['pileup_events'] >= 1
        _assert_agree(mapped, got0, got1)
    finally:
        ctx.close()


def test_watch_refusals(mapped):
    ctx = _native.Context(0)
    try:
        with pytest.raises(_native.NativeError) as err:
            ctx.pileup_watch([(0, k + 1) for k in range(_native.WATCH_MAXKEYS + 1)])
        assert '(-3)' in str(err.value)
        with pytest.raises(_native.NativeError):
            ctx.pileup_watch([(0, 0)])
        ctx.pileup_watch([(0, k + 1) for k in range(_native.WATCH_MAXKEYS)])   # the most allowed
        sam = '@SQ\tSN:a\n@SQ\tSN:b\nq\t0\ta\t1\t44\t4M\t*\t0\t0\tACGT\tFFFF\n'
        ctx.rows_load_sam(sam)
        with pytest.raises(_native.NativeError) as err:
            ctx.pileup(1, 0, [10, 10], only=[0])
        assert '(-3)' in str(err.value) and 'watch' in str(err.value)
        ctx.pileup(1, 0, [10, 10])
        counts, first = ctx.pileup_watch_fetch()
        assert counts.sum() == 4 and counts[0, 0, ord('F') - 32] == 1 and first[0, 0, ord('F') - 32] == 0
        # a sharded pileup does not exchange the histogram: refused while watching
        shard = Shard.__new__(Shard)
        with pytest.raises(RuntimeError, match='watched positions'):
            shard.pileup(ctx, 0)
        ctx.pileup_watch([])
        ctx.pileup(1, 0, [10, 10], only=[0])
    finally:
        ctx.close()


# ---- remap(debug_file_prefix=...) ----------------------------------------------
def _gz(path, mode='rb'):
    with gzip.open(path, mode) as f:
        return f.read()


def _run_remap(d, out, prefix):
    r1 = os.path.join(d, 'R1.fastq.gz')
    r2 = os.path.join(d, 'R2.fastq.gz')
    r2 = r2 if os.path.exists(r2) else None
    remap_csv = io.StringIO()
    rm.remap(r1, r2, io.StringIO(_gz(os.path.join(d, 'prelim.csv.gz'), 'rt')), remap_csv, gzip=True,
             work_path=str(out), debug_file_prefix=prefix)
    return remap_csv.getvalue()


@pytest.fixture(scope='module')
def debug_runs(golden_dir, tmp_path_factory):
    """Every debug_files case through remap(debug_file_prefix=...), once."""
    runs = {}
    for case in FILE_CASES:
        out = tmp_path_factory.mktemp(case)
        remap_text = _run_remap(os.path.join(golden_dir, 'e2e', case), out, str(out / 'dbg'))
        runs[case] = (out, remap_text)
    return runs


@pytest.mark.parametrize('case', FILE_CASES)
def test_debug_files_equal_the_reference(golden_dir, debug_runs, case):
    out, remap_text = debug_runs[case]
    want_dir = os.path.join(golden_dir, 'debug_files', case)
    want = sorted(n[:-3] for n in os.listdir(want_dir) if n.startswith('remap'))
    assert sorted(os.listdir(out)) == ['dbg_' + n for n in want]        # and no other file
    for n in want:
        assert (out / ('dbg_' + n)).read_bytes() == _gz(os.path.join(want_dir, n + '.gz')), n
    assert remap_text == _gz(os.path.join(golden_dir, 'e2e', case, 'remap.csv.gz'), 'rt')


def test_no_prefix_writes_nothing(golden_dir, tmp_path):
    (tmp_path / 'kept.txt').write_text('x')
    text = _run_remap(os.path.join(golden_dir, 'e2e', 'micro_2070A-PR'), tmp_path, None)
    assert sorted(os.listdir(tmp_path)) == ['kept.txt']
    assert text == _gz(os.path.join(golden_dir, 'e2e', 'micro_2070A-PR', 'remap.csv.gz'), 'rt')


@pytest.mark.parametrize('case', FILE_CASES)
def test_each_pass_rebuilds_the_next_reference(golden_dir, debug_runs, case):
    """The loop closed: pass n's SAM file through sam_to_conseqs, as remap()
    calls build_conseqs (remap.py:576-581), is the FASTA pass n + 1 mapped
    to; the last pass's is the reference's own answer."""
    out, _text = debug_runs[case]
    last = json.loads(_gz(os.path.join(golden_dir, 'debug_files', case, 'last_conseqs.json.gz'), 'rt'))
    for n in range(1, last['passes'] + 1):
        with open(out / 'dbg_remap{}_debug.sam'.format(n)) as f:
            got = rm.sam_to_conseqs(f, CONSENSUS_Q_CUTOFF, seeds=SEEDS, is_filtered=True,
                                    filter_coverage=5)
        if n < last['passes']:
            want = (out / 'dbg_remap{}_debug_ref.fasta'.format(n + 1)).read_text()
            assert ''.join('>%s\n%s\n' % item for item in got.items()) == want, n
        else:
            assert list(got.items()) == list(last['conseqs'].items())
    if last['passes'] == 1:
        path = str(out / 'dbg_remap1_debug.sam')
        assert rm.build_conseqs(path, seeds=SEEDS, is_filtered=True, filter_coverage=5) == last['conseqs']


def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_two_ranks_write_the_same_debug_files(golden_dir, tmp_path):
    case = 'syn_unpaired300'
    d = os.path.join(golden_dir, 'e2e', case)
    base = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
                MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    worker = os.path.join(HERE, 'gpu_debug_files_worker.py')
    procs = [subprocess.Popen([sys.executable, worker, d, str(tmp_path)],
                              env=dict(base, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=240))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert codes == [0, 0]
    want_dir = os.path.join(golden_dir, 'debug_files', case)
    want = sorted(n[:-3] for n in os.listdir(want_dir) if n.startswith('remap'))
    made = sorted(n for n in os.listdir(tmp_path) if n.startswith('dbg_'))
    assert made == ['dbg_' + n for n in want]
    for n in want:
        assert (tmp_path / ('dbg_' + n)).read_bytes() == _gz(os.path.join(want_dir, n + '.gz')), n
    assert (tmp_path / 'remap.csv').read_text() == _gz(os.path.join(d, 'remap.csv.gz'), 'rt')


# ---- the resident shortcuts survive a sam_to_conseqs call ----------------------
def test_chain_keeps_its_resident_sources(golden_dir, tmp_path):
    case = 'syn_pol_indel'
    d = os.path.join(golden_dir, 'e2e', case)
    r1, r2 = os.path.join(d, 'R1.fastq.gz'), os.path.join(d, 'R2.fastq.gz')
    prelim, remap_csv, aligned = tmp_path / 'prelim.csv', tmp_path / 'remap.csv', tmp_path / 'aligned.csv'
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    with open(prelim) as f, open(remap_csv, 'w') as out:
        rm.remap(r1, r2, f, out, gzip=True, work_path=str(tmp_path), debug_file_prefix=str(tmp_path / 'dbg'))
    # mh_rows_load replaces the context's row table and the pileup, not the
    # resident reads and records sam2aln() takes remap.csv's rows from
    with open(tmp_path / 'dbg_remap1_debug.sam') as f:
        reports = {('HIV1B-pol-seed', 900): None}
        conseqs = rm.sam_to_conseqs(f, CONSENSUS_Q_CUTOFF, debug_reports=reports, seeds=SEEDS)
    assert list(conseqs) == ['HIV1B-pol-seed'] and reports['HIV1B-pol-seed', 900]
    with open(remap_csv) as f, open(aligned, 'w') as out:
        s2a.sam2aln(f, out)
    assert aligned.read_text() == _gz(os.path.join(d, 'aligned.csv.gz'), 'rt')
    outs = {k: tmp_path / (k + '.csv') for k in ('nuc', 'amino', 'coord_ins', 'conseq', 'failed', 'coverage')}
    hs = {k: open(p, 'w') for k, p in outs.items()}
    with open(aligned) as f:
        a2c.aln2counts(f, hs['nuc'], hs['amino'], hs['coord_ins'], hs['conseq'],
                       failed_align_csv=hs['failed'], coverage_summary_csv=hs['coverage'])
    for h in hs.values():
        h.close()
    for k, p in outs.items():
        assert p.read_text() == _gz(os.path.join(d, 'a2c_{}.csv.gz'.format(k)), 'rt'), k
    assert (session.stats['prelim_source'], session.stats['sam2aln_source'],
            session.stats['aln2counts_source']) == ('device', 'device', 'device')

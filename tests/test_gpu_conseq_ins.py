"""sam2aln's merged insertions on the device (k_s2a_ins_rec, k_s2a_ins_merge,
k_s2a_ins_tab behind mh_sam2aln_conseq_ins; micall_amd.sam2aln(conseq_ins_csv=))
against tests/ins_oracle.py, byte for byte: the hand-written cases, every
golden remap.csv through the text, file and resident routes, several
q-cutoffs in one call, synthetic texts that grow the table, pile every unit
on one key, leave most units out of the unit list, or hold one long or many
short insertions, the refusal of a '-', and a two-rank job."""
import gzip
import io
import json
import os
import random
import socket
import subprocess
import sys

import pytest

import ins_cases
import ins_oracle
from micall_amd import _native, session
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
OUTPUTS = ('aligned.csv', 'insert.csv', 'failed.csv')
HEAD_ONLY = 'refname,qcut,pos,insert,count\n'
NEW_KERNELS = ('k_s2a_ins_rec', 'k_s2a_ins_merge', 'k_s2a_ins_tab', 'k_s2a_ins_group')
_WANT = {}


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _golden(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.gz'), 'rt') as f:
        return f.read()


def _want(case, cuts=(15,)):
    """The oracle's conseq_ins.csv of a golden remap.csv, computed once."""
    key = case, tuple(cuts)
    if key not in _WANT:
        _WANT[key] = ins_oracle.conseq_ins(_golden(case, 'remap.csv'), cuts)
    return _WANT[key]


def _call(remap_handle, tmp_path, tag, **kw):
    """sam2aln() to files: (aligned, insert, failed, conseq_ins) texts."""
    paths = [tmp_path / '{}_{}'.format(tag, n) for n in OUTPUTS + ('conseq_ins.csv',)]
    handles = [open(p, 'w') for p in paths]
    try:
        s2a.sam2aln(remap_handle, *handles[:3], conseq_ins_csv=handles[3], **kw)
    finally:
        for h in handles:
            h.close()
    return tuple(p.read_text() for p in paths)


def _check_counts(ctx, text, cuts):
    """sam2aln_ins_counts() is the per-position sum of the text's rows."""
    ids, cut, pos, cnt = ctx.sam2aln_ins_counts()
    want = ins_oracle.totals(text)
    assert sorted(zip((cuts[k] for k in cut.tolist()), pos.tolist(), cnt.tolist())) == \
        sorted((c, p, n) for (_, c, p), n in want.items())
    assert len(ids) == len(want)


# ---------------------------------------------------------------------------
# the hand-written cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ins_cases.CASES))
def test_hand_written_case(ctx, name):
    rows, cuts, want = ins_cases.CASES[name]
    ctx.sam2aln_csv(ins_cases.text(rows), q_cutoffs=cuts)
    got = ctx.sam2aln_conseq_ins()
    assert got == ins_cases.expected_text(want)
    _check_counts(ctx, got, cuts)


def test_combined_cases(ctx):
    rows, want = ins_cases.combined()
    text = ins_cases.text(rows)
    ctx.profile(True)
    try:
        ctx.sam2aln_csv(text)
        assert ctx.sam2aln_conseq_ins() == ins_cases.expected_text(want) == ins_oracle.conseq_ins(text)
        assert ctx.sam2aln_conseq_ins() == ins_cases.expected_text(want)
        _check_counts(ctx, ins_cases.expected_text(want), [15])
        # asked three times: counted once
        assert [ctx.profile_get(k)[1] for k in NEW_KERNELS] == [1, 1, 1, 1]
    finally:
        ctx.profile(False)


# ---------------------------------------------------------------------------
# the goldens, text and file routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', E2E)
def test_golden_text_and_file_routes(case, tmp_path):
    """Byte-equal to the oracle by both routes (the header alone where the
    oracle says so), and the three other outputs of the same call are the
    goldens."""
    text = _golden(case, 'remap.csv')
    golden = tuple(_golden(case, n) for n in OUTPUTS)
    session.stats.pop('sam2aln_source', None)
    outs = [io.StringIO() for _ in range(4)]
    s2a.sam2aln(io.StringIO(text), *outs[:3], conseq_ins_csv=outs[3])
    assert tuple(o.getvalue() for o in outs[:3]) == golden
    assert outs[3].getvalue() == _want(case)
    path = tmp_path / 'remap.csv'
    path.write_text(text)
    with open(path) as f:
        got = _call(f, tmp_path, 'file')
    assert got[:3] == golden
    assert got[3] == _want(case)
    assert session.stats['sam2aln_source'] == 'csv'


def test_goldens_exercise_the_pass():
    assert sum(1 for case in E2E if _want(case) != HEAD_ONLY) == 7
    assert _want('syn_pol_indel').count('\n') - 1 == 32
    assert _want('syn_noseed') == HEAD_ONLY


# ---------------------------------------------------------------------------
# several cutoffs in one call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['c1_example', 'syn_pol_indel'])
def test_several_cutoffs(ctx, case):
    text = _golden(case, 'remap.csv')
    cuts = [0, 10, 15]
    ctx.sam2aln_csv(text, q_cutoffs=cuts)
    three = ctx.sam2aln_conseq_ins()
    assert three == _want(case, cuts)
    _check_counts(ctx, three, cuts)
    rows = three.splitlines(True)[1:]
    for c in cuts:
        ctx.sam2aln_csv(text, q_cutoffs=[c])
        # each cutoff's rows of the joint call are the single call's (the
        # joint call is the oracle's above, which takes the cutoffs one by one)
        single = ctx.sam2aln_conseq_ins().splitlines(True)[1:]
        assert single and single == [r for r in rows if r.split(',')[-4] == str(c)]


# ---------------------------------------------------------------------------
# the resident route
# ---------------------------------------------------------------------------
def _chain_to_remap(case, tmp_path):
    """prelim_map to a file, remap to files, as bin/micall chains them."""
    r1 = os.path.join(E2E_DIR, case, 'R1.fastq.gz')
    r2 = os.path.join(E2E_DIR, case, 'R2.fastq.gz')
    r2 = r2 if os.path.exists(r2) else None
    prelim = tmp_path / 'prelim.csv'
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    remap_csv = tmp_path / 'remap.csv'
    with open(prelim) as f, open(remap_csv, 'w') as out, open(tmp_path / 'counts.csv', 'w') as cn:
        rm.remap(r1, r2, f, out, cn, gzip=True, work_path=str(tmp_path))
    return remap_csv


@pytest.mark.parametrize('case', ['syn_pol_indel', 'c1_example', 'syn_unpaired300'])
def test_resident_route(case, tmp_path, monkeypatch):
    """prelim_map -> remap -> sam2aln(conseq_ins_csv=) in one process: the
    rows k_s2a_stage built feed the pass, and the result is the oracle's on
    the remap.csv written and the file route's."""
    remap_csv = _chain_to_remap(case, tmp_path)
    with open(remap_csv) as f:
        got = _call(f, tmp_path, 'dev')
    assert session.stats['sam2aln_source'] == 'device'
    assert got[3] == ins_oracle.conseq_ins(remap_csv.read_text())
    assert got[3] != HEAD_ONLY
    assert got[:3] == tuple(_golden(case, n) for n in OUTPUTS)
    monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    with open(remap_csv) as f:
        again = _call(f, tmp_path, 'file')
    assert session.stats['sam2aln_source'] == 'csv'
    assert again == got


# ---------------------------------------------------------------------------
# synthetic texts
# ---------------------------------------------------------------------------
def _random_insert(rng, n):
    seq = ''.join(rng.choice('ACGT') for _ in range(n))
    qual = ''.join(rng.choice('I:51/#') if rng.random() < 0.25 else 'I' for _ in range(n))
    return seq, qual


def test_spread_keys_grow_the_table(ctx):
    """4096 pairs with random 1-12-base insertions at random keys over a 9 kb
    reference, about a third with both mates at one key, qualities on both
    sides of the cutoff: thousands of distinct (key, string) entries."""
    rng = random.Random(11)
    rows = []
    for k in range(4096):
        p1 = rng.randint(1, 9000)
        a1, a2 = rng.randint(4, 20), rng.randint(4, 20)
        if rng.random() < 0.34:
            p2, b2 = p1, a1                  # both mates insert after p1 - 1 + a1
        else:
            p2, b2 = p1 + rng.randint(0, 12), rng.randint(4, 20)
        i1 = ('I',) + _random_insert(rng, rng.randint(1, 12))
        i2 = ('I',) + (i1[1:] if rng.random() < 0.3 else _random_insert(rng, rng.randint(1, 12)))
        rows += [ins_cases.read('q%d' % k, ins_cases.FWD, 'ref9k', p1, 'M%d' % a1, i1, 'M%d' % a2),
                 ins_cases.read('q%d' % k, ins_cases.REV, 'ref9k', p2, 'M%d' % b2, i2, 'M%d' % a2)]
    text = ins_cases.text(rows)
    counts, tallies = ins_oracle.counts(text)
    want = ins_oracle.to_text(ins_oracle.ordered(counts))
    assert want.count('\n') - 1 > 2000
    assert tallies['both'] > 800 and 'N' in want
    ctx.sam2aln_csv(text)
    got = ctx.sam2aln_conseq_ins()
    assert got == want
    _check_counts(ctx, got, [15])


def test_identical_pairs_pile_on_one_key(ctx):
    """4096 copies of one pair with one insertion, the amplicon case: one
    row with count 4096."""
    rows = []
    for k in range(4096):
        rows += [ins_cases.read('q%d' % k, ins_cases.FWD, 'amp', 100, 'M20', ('I', 'GAT'), 'M10'),
                 ins_cases.read('q%d' % k, ins_cases.REV, 'amp', 110, 'M10', ('I', 'GAT'), 'M20')]
    text = ins_cases.text(rows)
    want = ins_cases.expected_text([['amp', 15, 119, 'GAT', 4096]])
    assert ins_oracle.conseq_ins(text) == want
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_conseq_ins() == want


def test_unit_list_leaves_most_units_out(ctx):
    """9000 unpaired reads over two references, one in seven with an I op:
    the unit list is a fraction of the units and its last wave group is
    partly filled."""
    rng = random.Random(9)
    rows = []
    for k in range(9000):
        pieces = ['M12', ('I', rng.choice(['A', 'CG', 'TTT'])), 'M8'] if k % 7 == 3 else ['M20']
        rows.append(ins_cases.read('u%d' % k, ins_cases.UNPAIRED, 'refB' if k % 3 else 'refA',
                                   rng.randint(1, 300), *pieces))
    text = ins_cases.text(rows)
    want = ins_oracle.conseq_ins(text)
    assert sum(int(r.rsplit(',', 1)[1]) for r in want.splitlines()[1:]) == 9000 // 7 + (9000 % 7 > 3)
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_conseq_ins() == want


def test_one_long_insertion(ctx):
    """300 inserted bases in a 600-base read: several times a wave's 64
    lanes; the mate carries the first 200 of them."""
    rng = random.Random(3)
    seq = ''.join(rng.choice('ACGT') for _ in range(300))
    rows = [ins_cases.read('long', ins_cases.FWD, 'R1', 50, 'M150', ('I', seq), 'M150'),
            ins_cases.read('long', ins_cases.REV, 'R1', 100, 'M100', ('I', seq[:200]), 'M150')]
    assert len(rows[0][9]) == 600
    text = ins_cases.text(rows)
    want = ins_cases.expected_text([['R1', 15, 199, seq, 1]])
    assert ins_oracle.conseq_ins(text) == want
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_conseq_ins() == want


def test_many_insertions_in_one_read(ctx):
    """40 separate 1-base insertions in one read: 40 records of one unit."""
    pieces = ['M3']
    for k in range(40):
        pieces += [('I', 'ACGT'[k % 4]), 'M3']
    rows = [ins_cases.read('many', ins_cases.UNPAIRED, 'R1', 1, *pieces)]
    text = ins_cases.text(rows)
    want = ins_cases.expected_text([['R1', 15, 3 * (k + 1), 'ACGT'[k % 4], 1] for k in range(40)])
    assert ins_oracle.conseq_ins(text) == want
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_conseq_ins() == want


# ---------------------------------------------------------------------------
# refusal, and calls that do not ask
# ---------------------------------------------------------------------------
def test_a_dash_is_refused_by_read_name(ctx):
    """An inserted '-' is refused with the read's name; the call's other
    outputs and the next call work."""
    rows = [ins_cases.read('fine', ins_cases.UNPAIRED, 'R1', 10, 'M4', ('I', 'GG'), 'M4'),
            ins_cases.read('dashed', ins_cases.UNPAIRED, 'R1', 10, 'M4', ('I', 'G-'), 'M4')]
    text = ins_cases.text(rows)
    with pytest.raises(ins_oracle.Refused, match='dashed'):
        ins_oracle.conseq_ins(text)
    ctx.sam2aln_csv(text)
    with pytest.raises(_native.NativeError, match='dashed'):
        ctx.sam2aln_conseq_ins()
    with pytest.raises(_native.NativeError, match='dashed'):
        ctx.sam2aln_ins_counts()
    assert ctx.sam2aln_output('failed') == 'qname,cause\n'
    assert ctx.sam2aln_output('aligned').count('\n') == 2
    assert ctx.sam2aln_output('insert').count('\n') == 3
    rows, cuts, want = ins_cases.CASES['both_disagree']
    ctx.sam2aln_csv(ins_cases.text(rows), q_cutoffs=cuts)
    assert ctx.sam2aln_conseq_ins() == ins_cases.expected_text(want)


def test_a_call_that_does_not_ask_runs_no_new_kernel(ctx):
    """A call without conseq_ins gives the goldens, launches none of the new
    kernels and runs the merge once."""
    text = _golden('syn_pol_indel', 'remap.csv')
    ctx.profile(True)
    try:
        ctx.sam2aln_csv(text)
        got = tuple(ctx.sam2aln_output(w) for w in ('aligned', 'insert', 'failed'))
        assert [ctx.profile_get(k)[1] for k in NEW_KERNELS] == [0, 0, 0, 0]
        assert ctx.profile_get('k_s2a_merge')[1] == 1
        assert ctx.sam2aln_conseq_ins() == _want('syn_pol_indel')
        assert [ctx.profile_get(k)[1] for k in NEW_KERNELS] == [1, 1, 1, 1]
        assert ctx.profile_get('k_s2a_merge')[1] == 1
    finally:
        ctx.profile(False)
    assert got == tuple(_golden('syn_pol_indel', n) for n in OUTPUTS)


def test_no_call_no_insertions():
    c = _native.Context(0)
    try:
        with pytest.raises(_native.NativeError):
            c.sam2aln_conseq_ins()
        with pytest.raises(_native.NativeError):
            c.sam2aln_ins_counts()
    finally:
        c.close()


# ---------------------------------------------------------------------------
# two ranks on one GPU
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
def test_two_ranks(tmp_path):
    """syn_pol_indel's remap.csv over two ranks (gloo): one cutoff takes the
    sharded route, every rank counting its own units; three cutoffs take the
    rank-0 route.  Both give the oracle's file."""
    root = tmp_path / 'job'
    root.mkdir()
    (root / 'remap.csv').write_text(_golden('syn_pol_indel', 'remap.csv'))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, 'gpu_ins_worker.py'), '--dir', str(root)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=500) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0]
    stats = [json.load(open(root / ('rank%d.json' % r))) for r in range(2)]
    assert all(s['one'].get('mode') == 'sharded' for s in stats), stats
    assert all(s['three'].get('mode') != 'sharded' for s in stats), stats
    assert all(s['one']['units'] > 0 for s in stats), stats
    assert (root / 'one_conseq_ins.csv').read_text() == _want('syn_pol_indel')
    assert (root / 'three_conseq_ins.csv').read_text() == _want('syn_pol_indel', [0, 10, 15])
    assert (root / 'one_aligned.csv').read_text() == _golden('syn_pol_indel', 'aligned.csv')

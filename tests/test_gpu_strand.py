"""sam2aln's strand support on the device (k_s2a_strand, k_s2a_strand_scan
behind mh_sam2aln_strand; micall_amd.sam2aln(strand_csv=)) against
tests/strand_oracle.py, byte for byte: the hand-written cases, every golden
remap.csv through the text, file and resident routes, several cutoffs in one
pass, synthetic texts that pile a block's adds on one address, spread them
past its LDS window or cross what a 16-bit counter holds, the caps,
aln2counts' ten columns, and a two-rank job.  The device's own strand.csv
also reproduces the base counts of the reference-generated aligned.csv."""
import csv
import gzip
import io
import json
import os
import random
import socket
import subprocess
import sys

import pytest

import strand_cases as cases
import strand_oracle as oracle
from micall_amd import _native, session
from micall_amd import aln2counts as a2c
from micall_amd import sam2aln as s2a
from test_gpu_concordance import _chain_to_remap, _frames

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
OUTPUTS = ('aligned.csv', 'insert.csv', 'failed.csv')
HEAD = ','.join(cases.HEADER) + '\n'
KERNELS = ('k_s2a_strand', 'k_s2a_strand_scan')
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
    """The oracle's strand.csv of a golden remap.csv, computed once."""
    key = case, tuple(cuts)
    if key not in _WANT:
        _WANT[key] = oracle.strand(_golden(case, 'remap.csv'), cuts)
    return _WANT[key]


def _launches(ctx):
    return tuple(ctx.profile_get(k)[1] for k in KERNELS)


def _call(remap_handle, tmp_path, tag, **kw):
    """sam2aln() to files: (aligned, insert, failed, strand) texts."""
    paths = [tmp_path / '{}_{}'.format(tag, n) for n in OUTPUTS + ('strand.csv',)]
    handles = [open(p, 'w') for p in paths]
    try:
        s2a.sam2aln(remap_handle, *handles[:3], strand_csv=handles[3], **kw)
    finally:
        for h in handles:
            h.close()
    return tuple(p.read_text() for p in paths)


# ---------------------------------------------------------------------------
# the hand-written cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_hand_written_case(ctx, name):
    rows, cuts, want = cases.CASES[name]
    ctx.sam2aln_csv(cases.text(rows), q_cutoffs=cuts)
    text = ctx.sam2aln_strand()
    assert text == cases.expected_text(want, cuts)
    ids, cut, pos, cnt = ctx.sam2aln_strand_counts()
    assert [[q, p] + v for q, p, v in zip(cut.tolist(), pos.tolist(), cnt.tolist())] == \
        [[int(x) for x in line.split(',')[1:]] for line in text.splitlines()[1:]]
    assert len(set(ids.tolist())) == len({n for n, _, _ in want})


def test_combined_cases_asked_twice_counted_once(ctx):
    rows, want = cases.combined()
    ctx.profile(True)
    try:
        before = _launches(ctx)
        ctx.sam2aln_csv(cases.text(rows))
        assert ctx.sam2aln_strand() == cases.expected_text(want, [15])
        assert ctx.sam2aln_strand() == cases.expected_text(want, [15])
        ctx.sam2aln_strand_counts()
        assert _launches(ctx) == (before[0] + 1, before[1] + 1)
    finally:
        ctx.profile(False)


# ---------------------------------------------------------------------------
# the goldens, text and file routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', E2E)
def test_golden_text_and_file_routes(case, tmp_path):
    """Byte-equal to the oracle by both routes, the three other outputs of the
    same call are the goldens, and the device's own counts satisfy the
    identity with the reference's aligned.csv (no oracle of ours in it)."""
    text = _golden(case, 'remap.csv')
    golden = tuple(_golden(case, n) for n in OUTPUTS)
    session.stats.pop('sam2aln_source', None)
    outs = [io.StringIO() for _ in range(4)]
    s2a.sam2aln(io.StringIO(text), *outs[:3], strand_csv=outs[3])
    assert tuple(o.getvalue() for o in outs[:3]) == golden
    assert outs[3].getvalue() == _want(case)
    path = tmp_path / 'remap.csv'
    path.write_text(text)
    with open(path) as f:
        got = _call(f, tmp_path, 'file')
    assert got[:3] == golden
    assert got[3] == _want(case)
    assert session.stats['sam2aln_source'] == 'csv'
    assert oracle.called(oracle.rows(got[3])) == oracle.aligned_calls(golden[0])
    if case in ('syn_noseed', 'micro_2030A-V3LOOP', 'micro_2050A-V3LOOP'):
        assert got[3] == HEAD


# ---------------------------------------------------------------------------
# the resident route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ('c1_example', 'syn_pol_indel', 'syn_unpaired300', 'micro_2040A-HLA-B'))
def test_resident_route(case, tmp_path, monkeypatch):
    """prelim_map -> remap -> sam2aln(strand_csv=) in one process: the rows
    k_s2a_stage built feed the pass; equal to the oracle on the remap.csv
    written and to the file route."""
    remap_csv = _chain_to_remap(case, tmp_path)
    with open(remap_csv) as f:
        got = _call(f, tmp_path, 'dev')
    assert session.stats['sam2aln_source'] == 'device'
    assert got[3] == oracle.strand(remap_csv.read_text()) and got[3] != HEAD
    assert got[:3] == tuple(_golden(case, n) for n in OUTPUTS)
    monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    with open(remap_csv) as f:
        again = _call(f, tmp_path, 'file')
    assert session.stats['sam2aln_source'] == 'csv'
    assert again == got


# ---------------------------------------------------------------------------
# several cutoffs in one pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('cuts', ([0, 10, 15, 30], [30, 10]))
def test_several_cutoffs_one_pass(ctx, cuts):
    text = _golden('syn_pol_indel', 'remap.csv')
    ctx.profile(True)
    try:
        before = _launches(ctx)
        ctx.sam2aln_csv(text, q_cutoffs=cuts)
        got = ctx.sam2aln_strand()
        assert _launches(ctx) == (before[0] + 1, before[1] + 1)
    finally:
        ctx.profile(False)
    assert got == _want('syn_pol_indel', cuts)
    body = got.splitlines()[1:]
    for q in cuts:
        ctx.sam2aln_csv(text, q_cutoffs=[q])
        assert ctx.sam2aln_strand().splitlines()[1:] == [r for r in body if r.split(',')[1] == str(q)]


# ---------------------------------------------------------------------------
# synthetic texts
# ---------------------------------------------------------------------------
def _both_grids(ctx, text, want, cuts=(15,)):
    """With one block for every unit (mh_test_set_sam2aln) and with the library's own grid."""
    ctx.test_set_sam2aln(max_blocks=1)
    try:
        ctx.sam2aln_csv(text, q_cutoffs=list(cuts))
        assert ctx.sam2aln_strand() == want
    finally:
        ctx.test_set_sam2aln()
    ctx.sam2aln_csv(text, q_cutoffs=list(cuts))
    assert ctx.sam2aln_strand() == want


def _identical_pairs(n):
    """n copies of one 30M / 30M pair with a resolved mismatch; its strand.csv from one copy's."""
    pair = [cases.row('q', cases.FWD, 'amp', 100, '30M', edit={12: 'G'}),
            cases.row('q', cases.REV, 'amp', 110, '30M', quals={2: '5'})]
    one = oracle.count(cases.text(pair))
    assert len(one) == 40 and one['amp', 15, 112] == [0] * 6 + [1, 0, 0] + [0] * 6
    rows = []
    for k in range(n):
        rows += [['q%d' % k] + pair[0][1:], ['q%d' % k] + pair[1][1:]]
    return cases.text(rows), oracle.text({key: [n * x for x in v] for key, v in one.items()})


def test_identical_pairs_pile_on_one_address(ctx):
    text, want = _identical_pairs(4096)
    assert want == oracle.strand(text)
    _both_grids(ctx, text, want)


def _random_pairs(n, refs, span, seed, subs):
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        ref = refs[k % len(refs)] if k % 3 else refs[0]
        p1 = rng.randint(1, span)
        p2 = p1 + rng.randint(0, 40)
        l1, l2 = rng.randint(45, 80), rng.randint(45, 80)
        edits = [{rng.randrange(l): rng.choice('ACGTN') for _ in range(rng.randint(0, subs))} for l in (l1, l2)]
        quals = [{rng.randrange(l): rng.choice('#5?EFGI') for _ in range(6)} for l in (l1, l2)]
        flags = (cases.FWD, cases.REV) if k % 5 else (cases.REV1, cases.FWD2)
        rows += [cases.row('q%d' % k, flags[0], ref, p1, '%dM' % l1, edit=edits[0], quals=quals[0]),
                 cases.row('q%d' % k, flags[1], ref, p2, '%dM' % l2, edit=edits[1], quals=quals[1])]
    return cases.text(rows)


def test_window_larger_than_the_lds_tile(ctx):
    """4096 random pairs spread over a 9 kb reference with substitutions and
    mixed qualities, at one cutoff and at four (the window then holds a
    quarter of the positions): adds inside and outside the block's window."""
    text = _random_pairs(4096, ['ref9k'], 9000, 5, 12)
    want = oracle.strand(text)
    assert want.count('\n') > 8000
    _both_grids(ctx, text, want)
    cuts = [30, 2, 15, 22]
    _both_grids(ctx, text, oracle.strand(text, cuts), cuts)


def test_more_than_one_block_two_references(ctx):
    """9000 pairs on two references: several blocks, the last one partly
    filled, two windows side by side in the planes."""
    text = _random_pairs(9000, ['refB', 'refA'], 300, 9, 3)
    _both_grids(ctx, text, oracle.strand(text))


def test_a_block_cannot_wrap_its_16_bit_counters(ctx):
    """70 000 identical pairs and one block asked for: a block's 16-bit
    counters would wrap at 65 536, so the library splits the units over more
    blocks whatever the test asks.  Every count is 70 000."""
    text, want = _identical_pairs(70000)
    assert ',70000,' in want
    _both_grids(ctx, text, want)


# ---------------------------------------------------------------------------
# the caps, and calls that do not ask
# ---------------------------------------------------------------------------
def _far_apart(distance):
    return cases.text([cases.row('a', cases.FWD, 'ok_ref', 10, '10M'), cases.row('a', cases.REV, 'ok_ref', 12, '10M'),
                       cases.row('b', cases.FWD, 'far_ref', 1, '10M'), cases.row('b', cases.REV, 'far_ref', 3, '10M'),
                       cases.row('c', cases.FWD, 'far_ref', distance, '10M'),
                       cases.row('c', cases.REV, 'far_ref', distance, '10M')])


def _refused(ctx, match, n_cuts=1):
    """Both requests are refused; the call's other outputs and the next call work."""
    for ask in (ctx.sam2aln_strand, ctx.sam2aln_strand_counts):
        with pytest.raises(_native.NativeError, match=match):
            ask()
    assert ctx.sam2aln_output('failed') == 'qname,cause\n'
    assert ctx.sam2aln_output('aligned').count('\n') == 1 + 3 * n_cuts
    rows, cuts, want = cases.CASES['d_one_padding']
    ctx.sam2aln_csv(cases.text(rows), q_cutoffs=cuts)
    assert ctx.sam2aln_strand() == cases.expected_text(want, cuts)


def test_window_cap_refused_by_name(ctx):
    """Two pairs of one reference 2**26 + 100 positions apart: refused with
    the reference's name; the call's other outputs and the next call work."""
    ctx.sam2aln_csv(_far_apart((1 << 26) + 100))
    _refused(ctx, 'far_ref')


def test_byte_cap_refused(ctx):
    """1.2 M positions at eight cutoffs: 120 class planes and their compacted
    copies pass 2**30 bytes."""
    ctx.sam2aln_csv(_far_apart(1200000), q_cutoffs=[0, 5, 10, 15, 20, 25, 30, 35])
    _refused(ctx, 'bytes of counters', 8)
    ctx.sam2aln_csv(_far_apart(1200000))          # one cutoff fits
    assert ctx.sam2aln_strand().count('\n') == 1 + 12 + 12 + 10


def test_no_call_no_counts():
    c = _native.Context(0)
    try:
        for ask in (c.sam2aln_strand, c.sam2aln_strand_counts):
            with pytest.raises(_native.NativeError):
                ask()
    finally:
        c.close()


def test_a_call_that_does_not_ask_runs_no_strand_kernel(ctx):
    text = _golden('syn_pol_indel', 'remap.csv')
    ctx.profile(True)
    try:
        base = _launches(ctx)
        merges = ctx.profile_get('k_s2a_merge')[1]
        ctx.sam2aln_csv(text)
        assert ctx.sam2aln_strand() == _want('syn_pol_indel')
        assert _launches(ctx) == (base[0] + 1, base[1] + 1)
        ctx.sam2aln_csv(text)
        got = tuple(ctx.sam2aln_output(w) for w in ('aligned', 'insert', 'failed'))
        assert _launches(ctx) == (base[0] + 1, base[1] + 1)
        assert ctx.profile_get('k_s2a_merge')[1] == merges + 2
    finally:
        ctx.profile(False)
    assert got == tuple(_golden('syn_pol_indel', n) for n in OUTPUTS)


# ---------------------------------------------------------------------------
# aln2counts: the ten columns of nuc_detail.csv
# ---------------------------------------------------------------------------
def _nuc_detail(aligned_text, **kw):
    outs = [io.StringIO() for _ in range(5)]
    a2c.aln2counts(io.StringIO(aligned_text), *outs[:4], nuc_detail_csv=outs[4], **kw)
    return outs[4].getvalue()


def test_nuc_detail_columns():
    """With strand_csv every row of nuc_detail.csv ends with the ten fwd and
    rev counts of its consensus position, query.nuc.pos - reading frame (the
    frame from the oracle's Report), at its q-cutoff; 0 without an entry or a
    query position; without it the file is what it was."""
    aligned = _golden('c1_example', 'aligned.csv')
    strand = _want('c1_example')
    at = oracle.rows(strand)
    frames = _frames(aligned)
    plain = list(csv.reader(io.StringIO(_nuc_detail(aligned))))
    got = list(csv.reader(io.StringIO(_nuc_detail(aligned, strand_csv=io.StringIO(strand)))))
    ten = [k for k in range(15) if k % 3 != 2]
    want = [plain[0] + [cases.HEADER[3 + k] for k in ten]]
    for r in plain[1:]:
        seed, region, qcut, query = r[0], r[1], r[2], r[3]
        v = [0] * 15 if query == '' else at.get((seed, int(qcut), int(query) - frames[seed, region]), [0] * 15)
        want.append(r + [str(v[k]) for k in ten])
    assert got == want
    assert sum(1 for r in want[1:] if any(int(x) for x in r[-10:])) > 2000
    assert _nuc_detail(aligned) == _nuc_detail(aligned, strand_csv=None)
    every = _nuc_detail(aligned, conseq_ins_csv=io.StringIO('refname,qcut,pos,insert,count\n'),
                        concordance_csv=io.StringIO('refname,pos,overlap,mismatch,indel,nocall,unresolved\n'),
                        clipping_csv=io.StringIO('refname,pos,count\n'), strand_csv=io.StringIO(strand))
    assert every.splitlines()[0].endswith(',coverage,ins,overlap,mismatch,indel,A_fwd,A_rev,C_fwd,C_rev,'
                                          'G_fwd,G_rev,T_fwd,T_rev,del_fwd,del_rev')


# ---------------------------------------------------------------------------
# two ranks on one GPU
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
def test_two_ranks(tmp_path):
    """c1_example's remap.csv over two ranks (gloo): one cutoff takes the
    sharded route, every rank counting its own units; three cutoffs take the
    rank-0 route.  Both give the oracle's file."""
    root = tmp_path / 'job'
    root.mkdir()
    (root / 'remap.csv').write_text(_golden('c1_example', 'remap.csv'))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, 'gpu_strand_worker.py'), '--dir', str(root)],
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
    assert all(0 < s['one']['units'] < 9600 for s in stats), stats
    assert (root / 'one_strand.csv').read_text() == _want('c1_example')
    assert (root / 'three_strand.csv').read_text() == _want('c1_example', [0, 10, 15])
    assert (root / 'one_aligned.csv').read_text() == _golden('c1_example', 'aligned.csv')

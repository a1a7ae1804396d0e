"""sam2aln's soft-clip counts on the device (k_s2a_clip, k_s2a_clip_scan
behind mh_sam2aln_clipping; micall_amd.sam2aln(clipping_csv=)) against
tests/clip_oracle.py, byte for byte: the hand-written cases, every golden
remap.csv through the text, file and resident routes, synthetic texts that
spread a block's keys or pile them on one address, the window cap, and a
two-rank job."""
import gzip
import io
import json
import os
import random
import socket
import subprocess
import sys

import pytest

import clip_cases
import clip_oracle
from micall_amd import _native, session
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
OUTPUTS = ('aligned.csv', 'insert.csv', 'failed.csv')
HEAD_ONLY = 'refname,pos,count\n'
_WANT = {}


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _golden(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.gz'), 'rt') as f:
        return f.read()


def _want(case):
    """The oracle's clipping.csv of a golden remap.csv, computed once."""
    if case not in _WANT:
        _WANT[case] = clip_oracle.clipping(_golden(case, 'remap.csv'))[0]
    return _WANT[case]


def _call(remap_handle, tmp_path, tag, **kw):
    """sam2aln() to files: (aligned, insert, failed, clipping) texts."""
    paths = [tmp_path / '{}_{}'.format(tag, n) for n in OUTPUTS + ('clipping.csv',)]
    handles = [open(p, 'w') for p in paths]
    try:
        s2a.sam2aln(remap_handle, *handles[:3], clipping_csv=handles[3], **kw)
    finally:
        for h in handles:
            h.close()
    return tuple(p.read_text() for p in paths)


# ---------------------------------------------------------------------------
# the hand-written cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(clip_cases.CASES))
def test_hand_written_case(ctx, name):
    rows, want = clip_cases.CASES[name]
    ctx.sam2aln_csv(clip_cases.text(rows))
    assert ctx.sam2aln_clipping() == clip_cases.expected_text(want)
    ids, pos, cnt = ctx.sam2aln_clip_counts()
    assert sorted(zip(pos.tolist(), cnt.tolist())) == sorted((p, n) for (_, p), n in want.items())


def test_combined_cases(ctx):
    rows, want = clip_cases.combined()
    ctx.sam2aln_csv(clip_cases.text(rows))
    assert ctx.sam2aln_clipping() == clip_cases.expected_text(want)
    assert ctx.sam2aln_clipping() == clip_cases.expected_text(want)      # asked twice: counted once


# ---------------------------------------------------------------------------
# the goldens, text and file routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', E2E)
def test_golden_text_and_file_routes(case, tmp_path):
    """Byte-equal to the oracle by both routes (header alone for the empty
    cases), and the three other outputs of the same call are the goldens."""
    text = _golden(case, 'remap.csv')
    golden = tuple(_golden(case, n) for n in OUTPUTS)
    session.stats.pop('sam2aln_source', None)
    outs = [io.StringIO() for _ in range(4)]
    s2a.sam2aln(io.StringIO(text), *outs[:3], clipping_csv=outs[3])
    assert tuple(o.getvalue() for o in outs[:3]) == golden
    assert outs[3].getvalue() == _want(case)
    path = tmp_path / 'remap.csv'
    path.write_text(text)
    with open(path) as f:
        got = _call(f, tmp_path, 'file')
    assert got[:3] == golden
    assert got[3] == _want(case)
    assert session.stats['sam2aln_source'] == 'csv'
    if case in ('syn_noseed', 'micro_2030A-V3LOOP'):
        assert got[3] == HEAD_ONLY


def test_goldens_exercise_the_pass():
    assert _want('c1_example').count('\n') > 2000
    assert sum(1 for case in E2E if _want(case) != HEAD_ONLY) >= 7


def test_cutoffs_do_not_change_the_counts(ctx):
    text = _golden('c1_example', 'remap.csv')
    ctx.sam2aln_csv(text, q_cutoffs=[0, 10, 15])
    three = ctx.sam2aln_clipping()
    ctx.sam2aln_csv(text, q_cutoffs=[15])
    assert three == ctx.sam2aln_clipping() == _want('c1_example')


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


@pytest.mark.parametrize('case', ['c1_example', 'syn_pol_indel', 'syn_unpaired300'])
def test_resident_route(case, tmp_path, monkeypatch):
    """prelim_map -> remap -> sam2aln(clipping_csv=) in one process: the rows
    k_s2a_stage built feed the clip pass, and the counts are the oracle's on
    the remap.csv written and the file route's."""
    remap_csv = _chain_to_remap(case, tmp_path)
    with open(remap_csv) as f:
        got = _call(f, tmp_path, 'dev')
    assert session.stats['sam2aln_source'] == 'device'
    assert got[3] == clip_oracle.clipping(remap_csv.read_text())[0]
    assert got[3] != HEAD_ONLY
    assert got[:3] == tuple(_golden(case, n) for n in OUTPUTS)
    monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    with open(remap_csv) as f:
        again = _call(f, tmp_path, 'file')
    assert session.stats['sam2aln_source'] == 'csv'
    assert again == got


# ---------------------------------------------------------------------------
# synthetic texts: many keys per block, one key for all
# ---------------------------------------------------------------------------
def _pair(k, ref, p1, c1, p2, c2):
    return [clip_cases.row('q%d' % k, clip_cases.FWD, ref, p1, c1),
            clip_cases.row('q%d' % k, clip_cases.REV, ref, p2, c2)]


def test_spread_keys_overflow_the_block_table(ctx):
    """4096 pairs with their clip ends spread over a 9 kb reference.  One
    block of k_s2a_clip takes all 4096 units (256 threads x 16 units) and
    its LDS table has CLIP_SLOTS = 1024 slots, 8 probes each: the pairs' ~16
    thousand steps fall on several thousand distinct positions, so most of
    them overflow the table and go straight to the difference array."""
    rng = random.Random(5)
    rows = []
    for k in range(4096):
        p1 = rng.randint(10, 9000)
        p2 = p1 + rng.randint(-5, 30)
        c1 = '{}S{}M{}S'.format(rng.randint(0, 6), rng.randint(8, 25), rng.randint(0, 6)).replace('0S', '')
        c2 = '{}S{}M{}S'.format(rng.randint(0, 6), rng.randint(8, 25), rng.randint(0, 6)).replace('0S', '')
        rows += _pair(k, 'ref9k', p1, c1, p2, c2)
    text = clip_cases.text(rows)
    want, tallies = clip_oracle.clipping(text)
    assert want.count('\n') > 3 * 1024 and tallies['lost_to_mate'] > 500 and tallies['common'] > 100
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_clipping() == want


def test_identical_pairs_pile_on_one_address(ctx):
    """4096 copies of one pair, the amplicon case: every unit's steps fall on
    the same four addresses, and each counted position holds 4096."""
    rows = []
    for k in range(4096):
        rows += _pair(k, 'amp', 100, '3S20M', 110, '20M4S')
    text = clip_cases.text(rows)
    want = clip_cases.expected_text({('amp', p): 4096 for p in (97, 98, 99, 130, 131, 132, 133)})
    assert clip_oracle.clipping(text)[0] == want
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_clipping() == want


def test_more_than_one_block(ctx):
    """9000 unpaired reads: three blocks, the last one partly filled, two
    references whose windows sit side by side in the difference array."""
    rng = random.Random(9)
    rows = [clip_cases.row('u%d' % k, clip_cases.UNPAIRED, 'refB' if k % 3 else 'refA',
                           rng.randint(1, 300), '{}S12M{}S'.format(rng.randint(1, 4), rng.randint(1, 4)))
            for k in range(9000)]
    text = clip_cases.text(rows)
    ctx.sam2aln_csv(text)
    assert ctx.sam2aln_clipping() == clip_oracle.clipping(text)[0]


# ---------------------------------------------------------------------------
# the window cap, and calls that do not ask
# ---------------------------------------------------------------------------
def test_window_cap_refused_by_name(ctx):
    """Two reads of one reference 2**26 + 100 positions apart: refused with
    the reference's name; the call's other outputs and the next call work."""
    rows = [clip_cases.row('a', clip_cases.UNPAIRED, 'ok_ref', 10, '2S5M'),
            clip_cases.row('b', clip_cases.UNPAIRED, 'far_ref', 1, '2S5M'),
            clip_cases.row('c', clip_cases.UNPAIRED, 'far_ref', (1 << 26) + 100, '5M2S')]
    ctx.sam2aln_csv(clip_cases.text(rows))
    with pytest.raises(_native.NativeError, match='far_ref'):
        ctx.sam2aln_clipping()
    with pytest.raises(_native.NativeError, match='far_ref'):
        ctx.sam2aln_clip_counts()
    assert ctx.sam2aln_output('failed') == 'qname,cause\n'
    assert ctx.sam2aln_output('aligned').count('\n') == 4
    rows, want = clip_cases.CASES['both_ends']
    ctx.sam2aln_csv(clip_cases.text(rows))
    assert ctx.sam2aln_clipping() == clip_cases.expected_text(want)


def test_a_call_that_does_not_ask_runs_no_clip_kernel(ctx):
    """After a call with clipping, a call without it gives the goldens and
    launches neither new kernel (the context's kernel profile)."""
    text = _golden('syn_pol_indel', 'remap.csv')
    ctx.profile(True)
    try:
        ctx.sam2aln_csv(text)
        assert ctx.sam2aln_clipping() == _want('syn_pol_indel')
        assert ctx.profile_get('k_s2a_clip')[1] == 1 and ctx.profile_get('k_s2a_clip_scan')[1] == 1
        ctx.sam2aln_csv(text)
        got = tuple(ctx.sam2aln_output(w) for w in ('aligned', 'insert', 'failed'))
        assert ctx.profile_get('k_s2a_clip')[1] == 1 and ctx.profile_get('k_s2a_clip_scan')[1] == 1
        assert ctx.profile_get('k_s2a_merge')[1] == 2
    finally:
        ctx.profile(False)
    assert got == tuple(_golden('syn_pol_indel', n) for n in OUTPUTS)


def test_no_call_no_counts():
    c = _native.Context(0)
    try:
        with pytest.raises(_native.NativeError):
            c.sam2aln_clipping()
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
    """c1_example's remap.csv over two ranks (gloo): one cutoff takes the
    sharded route, every rank counting its own units; three cutoffs take the
    rank-0 route.  Both give the oracle's file."""
    root = tmp_path / 'job'
    root.mkdir()
    (root / 'remap.csv').write_text(_golden('c1_example', 'remap.csv'))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, 'gpu_clip_worker.py'), '--dir', str(root)],
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
    assert (root / 'one_clipping.csv').read_text() == _want('c1_example')
    assert (root / 'three_clipping.csv').read_text() == _want('c1_example')
    assert (root / 'one_aligned.csv').read_text() == _golden('c1_example', 'aligned.csv')

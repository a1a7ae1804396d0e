"""sam2aln's mate concordance on the device (k_s2a_conc, k_s2a_conc_scan behind
mh_sam2aln_concordance; micall_amd.sam2aln(concordance_csv=,
cycle_concordance_csv=)) against tests/concordance_oracle.py, byte for byte:
the hand-written cases, every golden remap.csv through the text, file and
resident routes, synthetic texts that pile a block's adds on one address or
spread them past its table, the window cap, aln2counts' three columns, and a
two-rank job."""
import csv
import gzip
import io
import itertools
import json
import os
import random
import socket
import subprocess
import sys

import pytest

import concordance_cases as cases
import concordance_oracle as oracle
import og_aln2counts as og
from micall_amd import _native, session
from micall_amd import aln2counts as a2c
from micall_amd import prelim_map as pm
from micall_amd import projects
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
OUTPUTS = ('aligned.csv', 'insert.csv', 'failed.csv')
HEADS = ('refname,pos,overlap,mismatch,indel,nocall,unresolved\n', 'read,by,value,compared,mismatch\n')
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
    """The oracle's two files of a golden remap.csv, computed once."""
    if case not in _WANT:
        _WANT[case] = oracle.concordance(_golden(case, 'remap.csv'))
    return _WANT[case]


def _both(ctx):
    return ctx.sam2aln_concordance(0), ctx.sam2aln_concordance(1)


def _call(remap_handle, tmp_path, tag, **kw):
    """sam2aln() to files: (aligned, insert, failed, concordance, cycle_concordance) texts."""
    paths = [tmp_path / '{}_{}'.format(tag, n) for n in OUTPUTS + ('concordance.csv', 'cycle.csv')]
    handles = [open(p, 'w') for p in paths]
    try:
        s2a.sam2aln(remap_handle, *handles[:3], concordance_csv=handles[3],
                    cycle_concordance_csv=handles[4], **kw)
    finally:
        for h in handles:
            h.close()
    return tuple(p.read_text() for p in paths)


# ---------------------------------------------------------------------------
# the hand-written cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_hand_written_case(ctx, name):
    rows, want_p, want_r = cases.CASES[name]
    ctx.sam2aln_csv(cases.text(rows))
    assert _both(ctx) == cases.expected_texts(want_p, want_r)
    ids, pos, cnt, reads = ctx.sam2aln_conc_counts()
    assert sorted(zip(pos.tolist(), cnt.tolist())) == sorted((p, n) for (_, p), n in want_p.items())
    assert sorted(reads.tolist()) == sorted([r, by == 'quality', v] + n for (r, by, v), n in want_r.items())


def test_combined_cases_asked_twice_counted_once(ctx):
    rows, want_p, want_r = cases.combined()
    ctx.profile(True)
    try:
        before = ctx.profile_get('k_s2a_conc')[1]
        ctx.sam2aln_csv(cases.text(rows))
        assert _both(ctx) == cases.expected_texts(want_p, want_r)
        assert _both(ctx) == cases.expected_texts(want_p, want_r)
        ctx.sam2aln_conc_counts()
        assert ctx.profile_get('k_s2a_conc')[1] == before + 1
        assert ctx.profile_get('k_s2a_conc_scan')[1] == before + 1
    finally:
        ctx.profile(False)


# ---------------------------------------------------------------------------
# the goldens, text and file routes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', E2E)
def test_golden_text_and_file_routes(case, tmp_path):
    """Byte-equal to the oracle by both routes (headers alone for the cases
    without a pair), and the three other outputs of the same call are the
    goldens."""
    text = _golden(case, 'remap.csv')
    golden = tuple(_golden(case, n) for n in OUTPUTS)
    session.stats.pop('sam2aln_source', None)
    outs = [io.StringIO() for _ in range(5)]
    s2a.sam2aln(io.StringIO(text), *outs[:3], concordance_csv=outs[3], cycle_concordance_csv=outs[4])
    assert tuple(o.getvalue() for o in outs[:3]) == golden
    assert (outs[3].getvalue(), outs[4].getvalue()) == _want(case)
    path = tmp_path / 'remap.csv'
    path.write_text(text)
    with open(path) as f:
        got = _call(f, tmp_path, 'file')
    assert got[:3] == golden
    assert got[3:] == _want(case)
    assert session.stats['sam2aln_source'] == 'csv'
    if case in ('syn_noseed', 'micro_2030A-V3LOOP', 'syn_unpaired300'):
        assert got[3:] == HEADS


def test_one_file_alone(tmp_path):
    """Either output without the other."""
    text = _golden('syn_pol_indel', 'remap.csv')
    for k in (0, 1):
        outs = [io.StringIO() for _ in range(4)]
        kw = {('concordance_csv', 'cycle_concordance_csv')[k]: outs[3]}
        s2a.sam2aln(io.StringIO(text), *outs[:3], **kw)
        assert outs[3].getvalue() == _want('syn_pol_indel')[k]


def test_cutoffs_do_not_change_the_counts(ctx):
    text = _golden('c1_example', 'remap.csv')
    ctx.sam2aln_csv(text, q_cutoffs=[0, 10, 15])
    three = _both(ctx)
    ctx.sam2aln_csv(text, q_cutoffs=[15])
    assert three == _both(ctx) == _want('c1_example')


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


NO_INSERTION = ('micro_2040A-HLA-B', 'micro_2090A-HCV', 'micro_2100A-HCV-1337B-V3LOOP')


def _paired_read_lengths(remap_text):
    """(longest paired read, longest paired read with an I op) of remap.csv text."""
    rows = [r for r in csv.DictReader(io.StringIO(remap_text)) if int(r['flag']) & 1 and r['cigar'] != '*']
    return (max([len(r['seq']) for r in rows], default=0),
            max([len(r['seq']) for r in rows if 'I' in r['cigar']], default=0))


@pytest.mark.parametrize('case', ('c1_example', 'syn_pol_indel', 'syn_unpaired300') + NO_INSERTION)
def test_resident_route(case, tmp_path, monkeypatch):
    """prelim_map -> remap -> sam2aln(concordance_csv=, cycle_concordance_csv=)
    in one process: the rows k_s2a_stage built feed the pass, and the counts
    are the oracle's on the remap.csv written and the file route's.  The
    resident rows keep a read's length on the host only where insert.csv
    quotes it; the NO_INSERTION cases have no I op in any paired row."""
    remap_csv = _chain_to_remap(case, tmp_path)
    if case in NO_INSERTION:
        longest, longest_ins = _paired_read_lengths(remap_csv.read_text())
        assert longest > 50 and longest_ins == 0
    with open(remap_csv) as f:
        got = _call(f, tmp_path, 'dev')
    assert session.stats['sam2aln_source'] == 'device'
    assert got[3:] == oracle.concordance(remap_csv.read_text())
    assert (got[3:] == HEADS) == (case == 'syn_unpaired300')
    assert got[:3] == tuple(_golden(case, n) for n in OUTPUTS)
    monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    with open(remap_csv) as f:
        again = _call(f, tmp_path, 'file')
    assert session.stats['sam2aln_source'] == 'csv'
    assert again == got


def _revcomp(seq):
    return seq[::-1].translate(str.maketrans('ACGT', 'TGCA'))


def test_resident_rows_whose_longest_read_has_no_insertion():
    """Resident rows of a mapping pass over 251-base pairs that fit the
    reference and 150-base pairs whose read 1 inserts three bases: the
    longest read with an I op is shorter than the longest read, and cycles up
    to 251 are counted.  Equal to the oracle on the rows as remap.csv prints
    them and to the text route on those rows."""
    pol = projects.load_default().seed_sequences()['HIV1B-pol-seed']
    rng = random.Random(21)
    names, seqs, quals = [], [], []
    for k in range(60):
        a = rng.randrange(100, len(pol) - 500)
        if k % 3:
            r1, r2 = pol[a:a + 251], _revcomp(pol[a + 149:a + 400])
        else:
            r1 = pol[a:a + 75] + 'GCA' + pol[a + 75:a + 147]
            r2 = _revcomp(pol[a + 60:a + 210])
        for r in (r1, r2):
            names.append('pair%d' % k)
            seqs.append(r)
            quals.append(''.join(rng.choice('5?FGI') for _ in r))
    ctx, ctx2 = _native.Context(0), _native.Context(0)
    try:
        ctx.index_build(['HIV1B-pol-seed'], [pol], 20)
        ctx.reads_load(seqs, quals, True, names=names)
        ctx.map(_native.params(_native.LOCAL))
        assert ctx.sam2aln_resident(['HIV1B-pol-seed'], q_cutoffs=[15]) == len(seqs) // 2
        text = ','.join(cases.HEADER) + '\n' + ctx.format_rows(1, 0, len(seqs))
        longest, longest_ins = _paired_read_lengths(text)
        assert longest == 251 and 0 < longest_ins < 251
        want = oracle.concordance(text)
        assert max(v for (_, by, v) in oracle.read_dict(want[1]) if by == 'cycle') > 200
        assert _both(ctx) == want
        ctx2.sam2aln_csv(text)
        assert _both(ctx2) == want
    finally:
        ctx.close()
        ctx2.close()


# ---------------------------------------------------------------------------
# synthetic texts: one key for all, many keys per block, several blocks
# ---------------------------------------------------------------------------
def test_identical_pairs_pile_on_one_address(ctx):
    """4096 copies of one pair with one mismatch, the amplicon case: every
    count of both files is 4096."""
    rows = []
    for k in range(4096):
        rows += [cases.row('q%d' % k, cases.FWD, 'amp', 100, '30M', edit={12: 'G'}),
                 cases.row('q%d' % k, cases.REV, 'amp', 110, '30M')]
    text = cases.text(rows)
    want = oracle.concordance(text)
    positions, reads = oracle.position_dict(want[0]), oracle.read_dict(want[1])
    assert len(positions) == 20 and positions['amp', 112] == [4096, 4096, 0, 0, 4096]
    assert all(v[0] == 4096 and v[1] in (0, 4096) for v in positions.values())
    assert all(v[0] % 4096 == 0 and v[1] in (0, 4096) for v in reads.values())
    ctx.sam2aln_csv(text)
    assert _both(ctx) == want


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
        rows += [cases.row('q%d' % k, cases.FWD, ref, p1, '%dM' % l1, edit=edits[0], quals=quals[0]),
                 cases.row('q%d' % k, cases.REV, ref, p2, '%dM' % l2, edit=edits[1], quals=quals[1])]
    return cases.text(rows)


def test_spread_keys_overflow_the_block_table(ctx):
    """4096 random pairs spread over a 9 kb reference with random
    substitutions.  With one block for all of them (mh_test_set_sam2aln) its
    table of 1024 slots, 8 probes each, takes a fraction of the ~8 thousand
    steps and several thousand discordant positions: the rest go straight to
    the arrays.  The library's own launch gives the same bytes."""
    text = _random_pairs(4096, ['ref9k'], 9000, 5, 12)
    want = oracle.concordance(text)
    sums = [sum(v[k] for v in oracle.position_dict(want[0]).values()) for k in range(5)]
    assert want[0].count('\n') > 8000 and sums[1] > 4096 and sums[3] > 1000 and sums[4] > 1000
    ctx.sam2aln_csv(text)
    assert _both(ctx) == want
    ctx.test_set_sam2aln(max_blocks=1)
    try:
        ctx.sam2aln_csv(text)
        assert _both(ctx) == want
    finally:
        ctx.test_set_sam2aln()


def test_more_than_one_block(ctx):
    """9000 pairs on two references: 141 blocks of 64 units, the last one
    partly filled, two windows side by side in the planes."""
    text = _random_pairs(9000, ['refB', 'refA'], 300, 9, 3)
    ctx.sam2aln_csv(text)
    assert _both(ctx) == oracle.concordance(text)


# ---------------------------------------------------------------------------
# the window cap, and calls that do not ask
# ---------------------------------------------------------------------------
def test_window_cap_refused_by_name(ctx):
    """Two pairs of one reference 2**26 + 100 positions apart: refused with
    the reference's name; the call's other outputs and the next call work."""
    rows = (cases._clean('a', 10, 10, 12, 10, ref='ok_ref')[0] + cases._clean('b', 1, 10, 3, 10, ref='far_ref')[0] +
            cases._clean('c', (1 << 26) + 100, 10, (1 << 26) + 100, 10, ref='far_ref')[0])
    ctx.sam2aln_csv(cases.text(rows))
    for ask in (lambda: ctx.sam2aln_concordance(0), lambda: ctx.sam2aln_concordance(1),
                ctx.sam2aln_conc_counts):
        with pytest.raises(_native.NativeError, match='far_ref'):
            ask()
    assert ctx.sam2aln_output('failed') == 'qname,cause\n'
    assert ctx.sam2aln_output('aligned').count('\n') == 4
    rows, want_p, want_r = cases.CASES['d_one_mate']
    ctx.sam2aln_csv(cases.text(rows))
    assert _both(ctx) == cases.expected_texts(want_p, want_r)


def test_a_call_that_does_not_ask_runs_no_concordance_kernel(ctx):
    """After a call with the concordance, a call without it gives the goldens
    and launches neither new kernel (the context's kernel profile)."""
    text = _golden('syn_pol_indel', 'remap.csv')
    ctx.profile(True)
    try:
        base = ctx.profile_get('k_s2a_conc')[1], ctx.profile_get('k_s2a_conc_scan')[1]
        merges = ctx.profile_get('k_s2a_merge')[1]
        ctx.sam2aln_csv(text)
        assert _both(ctx) == _want('syn_pol_indel')
        assert (ctx.profile_get('k_s2a_conc')[1], ctx.profile_get('k_s2a_conc_scan')[1]) == \
            (base[0] + 1, base[1] + 1)
        ctx.sam2aln_csv(text)
        got = tuple(ctx.sam2aln_output(w) for w in ('aligned', 'insert', 'failed'))
        assert (ctx.profile_get('k_s2a_conc')[1], ctx.profile_get('k_s2a_conc_scan')[1]) == \
            (base[0] + 1, base[1] + 1)
        assert ctx.profile_get('k_s2a_merge')[1] == merges + 2
    finally:
        ctx.profile(False)
    assert got == tuple(_golden('syn_pol_indel', n) for n in OUTPUTS)


def test_no_call_no_counts():
    c = _native.Context(0)
    try:
        with pytest.raises(_native.NativeError):
            c.sam2aln_concordance(0)
    finally:
        c.close()


# ---------------------------------------------------------------------------
# aln2counts: the three columns of nuc_detail.csv
# ---------------------------------------------------------------------------
def _nuc_detail(aligned_text, **kw):
    outs = [io.StringIO() for _ in range(5)]
    a2c.aln2counts(io.StringIO(aligned_text), *outs[:4], nuc_detail_csv=outs[4], **kw)
    return outs[4].getvalue()


def _frames(aligned):
    """{(seed, region): reading frame} as the oracle's Report maps them."""
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    frames = {}
    translate, seen = og.translate, {}

    def memo(*args):
        if args not in seen:
            seen[args] = translate(*args)
        return seen[args]
    og.translate = memo
    try:
        for _key, group in itertools.groupby(csv.DictReader(io.StringIO(aligned)),
                                             lambda r: (r['refname'], r['qcut'])):
            rep.read(group)
            for region in (rep.reports if rep.coordinate_refs else [rep.seed]):
                frames[rep.seed, region] = rep.reading_frames.get(region, 0) if rep.coordinate_refs else 0
    finally:
        og.translate = translate
    return frames


def test_nuc_detail_columns():
    """With concordance_csv every row of nuc_detail.csv ends with overlap,
    mismatch, indel of its consensus position, query.nuc.pos - reading frame
    (the frame from the oracle's Report), 0 without an entry or a query
    position; without it the file is what it was."""
    aligned = _golden('c1_example', 'aligned.csv')
    conc = _want('c1_example')[0]
    at = oracle.position_dict(conc)
    frames = _frames(aligned)
    plain = list(csv.reader(io.StringIO(_nuc_detail(aligned))))
    got = list(csv.reader(io.StringIO(_nuc_detail(aligned, concordance_csv=io.StringIO(conc)))))
    want = [plain[0] + ['overlap', 'mismatch', 'indel']]
    for r in plain[1:]:
        seed, region, query = r[0], r[1], r[3]
        three = [0, 0, 0] if query == '' else at.get((seed, int(query) - frames[seed, region]), [0, 0, 0])[:3]
        want.append(r + [str(n) for n in three])
    assert got == want
    assert sum(1 for r in want[1:] if int(r[-3]) > 0) > 2000 and any(int(r[-2]) for r in want[1:])
    assert _nuc_detail(aligned) == _nuc_detail(aligned, concordance_csv=None)
    with_ins = _nuc_detail(aligned, conseq_ins_csv=io.StringIO('refname,qcut,pos,insert,count\n'),
                           concordance_csv=io.StringIO(conc))
    assert with_ins.splitlines()[0].endswith(',coverage,ins,overlap,mismatch,indel')


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
    rank-0 route.  Both give the oracle's two files."""
    root = tmp_path / 'job'
    root.mkdir()
    (root / 'remap.csv').write_text(_golden('c1_example', 'remap.csv'))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, 'gpu_concordance_worker.py'),
                               '--dir', str(root)],
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
    for tag in ('one', 'three'):
        assert (root / (tag + '_concordance.csv')).read_text() == _want('c1_example')[0]
        assert (root / (tag + '_cycle.csv')).read_text() == _want('c1_example')[1]
    assert (root / 'one_aligned.csv').read_text() == _golden('c1_example', 'aligned.csv')

"""aln2counts' amino_detail.csv: amino.csv's rows with the codons it leaves out
(X, partial, del), ins, clip and coverage.

1. The device pass (k_a2c_detail through mh_a2c_codon_detail) against
   tests/amino_detail_oracle.py on rows loaded with a2c_load_rows: the
   hand-worked cases, bin and chunk edges, several groups, a full counter,
   random rows.
2. The file (SequenceReport.write_amino_detail, aln2counts(amino_detail_csv=))
   against rows built from the oracle's Report walk (oracle/og_aln2counts.py),
   amino_detail_oracle, clip_oracle and ins_oracle; aligned.csv, clipping.csv
   and conseq_ins.csv come from this build's sam2aln on the golden remap.csv."""
import csv
import gzip
import io
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import amino_detail_cases
import amino_detail_oracle as ado
import clip_oracle
import ins_oracle
from micall_amd import aln2counts as a2c
from micall_amd import sam2aln as s2a
from micall_amd import session

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_DIR = os.path.join(REPO, 'tests', 'golden', 'e2e')
SLOT = 2
SHIFTED = 'syn_pol_indel+1'
CASES = ['c1_example', 'syn_hiv3', 'syn_pol_indel', SHIFTED, 'syn_unpaired300']
PLAIN = ('nuc', 'amino', 'coord_ins', 'conseq')
X, PARTIAL, DEL, INS, CLIP, COVERAGE = range(26, 32)
_BUILT = {}
_EXPECTED = {}


# ---------------------------------------------------------------------------
# 1. the kernel against the oracle
# ---------------------------------------------------------------------------
def _extent(rows, frame):
    """The SeedAmino list length of a frame (aln2counts.py:155-160)."""
    return max([-(-(frame + off + len(seq)) // 3) for off, seq, _ in rows
                if -(-(frame + off + len(seq)) // 3) > off // 3] or [0])


def _load(groups, slot=SLOT):
    ctx = session.context()
    rows = [r for grp in groups for r in grp]
    first = [0]
    for grp in groups:
        first.append(first[-1] + len(grp))
    ctx.a2c_load_rows(slot, [r[1] for r in rows], [r[0] for r in rows], [r[2] for r in rows], first,
                      a2c._CODON_CHARS)
    return ctx


def _fetch(ctx, groups, slot=SLOT):
    """[group][frame] -> (codons, 3) tables of the slot, the extents checked."""
    out = []
    for g, rows in enumerate(groups):
        ncod = ctx.a2c_group(slot, g)['ncod']
        assert ncod == [_extent(rows, f) for f in range(3)]
        out.append([ctx.a2c_codon_detail(slot, g, f, ncod[f]) for f in range(3)])
    return out


def _check(groups):
    """Load the groups [(offset, seq, count)], compare every frame of every
    group with the oracle; returns the device tables."""
    ctx = _load(groups)
    got = _fetch(ctx, groups)
    for g, rows in enumerate(groups):
        cells = ado.tally(rows)
        for f in range(3):
            want = [[cells.get((f, j), {}).get(k, 0) for k in ado.CLASSES] for j in range(len(got[g][f]))]
            assert got[g][f].dtype == np.uint32
            assert got[g][f].tolist() == want, (g, f)
    return got


@pytest.mark.parametrize('name', sorted(amino_detail_cases.CASES))
def test_hand_worked_cases(name):
    rows, want = amino_detail_cases.CASES[name]
    got = _check([rows])[0]
    for f in range(3):
        assert got[f].tolist() == want[f], (name, f)


def test_padding_is_never_a_deletion():
    """Offsets 1, 2, 4, 5 with rows of 1 to 4 bases, and of 1 to 4 of the
    row's own '-': a '-' of the padding never makes a del, and where
    offset % 3 + frame >= 3 the first codon is blank."""
    for off in (1, 2, 4, 5):
        for n in (1, 2, 3, 4):
            got = _check([[(off, 'ACGT'[:n], 3)]])[0]
            assert all(int(t[:, 2].sum()) == 0 for t in got)
            for f in range(3):
                if off % 3 + f >= 3:
                    assert got[f][off // 3].tolist() == [0, 0, 0]
            dashes = _check([[(off, '-' * n, 3)]])[0]
            for f in range(3):
                # a deletion only where three of the row's own '-' fill a codon
                assert int(dashes[f][:, 2].sum()) == (3 if n >= 3 and (off + f) % 3 in ((0,) if n == 3 else (0, 2))
                                                      else 0)
                assert int(dashes[f][:, :2].sum()) == 0


def test_bin_edges():
    """Codons 20 | 21 and 41 | 42 are the last of one 21-codon bin and the
    first of the next; one row reaches over three bins."""
    rng = random.Random(3)
    long_row = ''.join(rng.choice('ACGTN-n') for _ in range(3 * 44 + 1))
    for rows in ([(60, 'ANA---', 2)], [(123, '---ANA', 3), (124, 'A-', 1)],
                 [(58, long_row, 5)],
                 [(60, 'ANA---', 2), (123, '---ANA', 3), (58, long_row, 5), (0, 'NNN' * 50, 7)]):
        got = _check([rows])[0]
        assert sum(int(t.sum()) for t in got) > 0
    got = _check([[(60, 'ANA---', 2)]])[0]
    assert got[0][20].tolist() == [2, 0, 0] and got[0][21].tolist() == [0, 0, 2]


def _distinct(n, rng, length=12):
    seen, rows = set(), []
    while len(rows) < n:
        row = rng.randrange(0, 50), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(1, length)))
        if row not in seen:
            seen.add(row)
            rows.append(row + (rng.randint(1, 9),))
    return rows


@pytest.mark.parametrize('n', [1025, 2049])
def test_chunk_edges(n):
    """More rows in one bin than a block takes (1024): the chunks' counters
    meet in the same cells."""
    _check([_distinct(n, random.Random(n))])


def test_two_groups_with_different_extents():
    rng = random.Random(11)
    groups = [[(0, 'ANACTN', 4), (2, 'AC---GT', 1)],
              [(200, ''.join(rng.choice('ACGTN-n') for _ in range(150)), 3), (7, 'N-NNNN', 2)],
              [(1, 'A', 1)]]
    got = _check(groups)
    assert [len(t) for t in got[0]] != [len(t) for t in got[1]]


def test_a_counter_fills_up():
    """The counts of one cell add up to 2**32 - 1 (a group's counts may)."""
    got = _check([[(0, 'ANA', 2 ** 32 - 2), (0, 'ANC', 1)]])[0]
    assert got[0][0].tolist() == [2 ** 32 - 1, 0, 0]


def test_nothing_to_count():
    """Rows whose codons are all letters or blank: every counter is zero."""
    got = _check([[(0, 'nnnnnn', 3), (3, 'nnn', 2)]])[0]
    assert [int(t.sum()) for t in got] == [0, 0, 0] and [len(t) for t in got] == [2, 3, 3]
    assert int(_check([[(0, 'CTGGCTAAA', 3)]])[0][0].sum()) == 0


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_rows(seed):
    rng = random.Random(seed)
    rows = [(rng.randint(0, 70), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(1, 200))),
             rng.randint(1, 1000)) for _ in range(300)]
    got = _check([rows])[0]
    assert all(int(t[:, k].sum()) > 0 for t in got for k in range(3))


def test_other_requests_on_the_slot_change_nothing():
    """a2c_counts returns what it returned before the detail pass; the
    detail is the same before and after a2c_inserts / a2c_variants."""
    rng = random.Random(5)
    rows = [(rng.randint(0, 30), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(20, 90))),
             rng.randint(1, 9)) for _ in range(200)] + [(0, 'ACGT' * 20, 2), (3, 'TTGCA' * 12, 1)]
    ctx = _load([rows])
    ncod = ctx.a2c_group(SLOT, 0)['ncod']
    before = [[a.copy() for a in ctx.a2c_counts(SLOT, 0, f, ncod[f])] for f in range(3)]
    detail = _fetch(ctx, [rows])[0]
    after = [ctx.a2c_counts(SLOT, 0, f, ncod[f]) for f in range(3)]
    assert all((a == b).all() for fa, fb in zip(before, after) for a, b in zip(fa, fb))
    assert ctx.a2c_inserts(SLOT, 0, 0, [4], [7])
    ctx.a2c_variants(SLOT, 0, [30], [60], [10], [5])
    again = _fetch(ctx, [rows])[0]
    assert all((a == b).all() for a, b in zip(detail, again))
    assert sum(int(t.sum()) for t in detail) > 0


def test_bad_requests_are_refused():
    from micall_amd import _native
    ctx = _load([[(0, 'ANA', 1)]])
    for g, frame in ((1, 0), (-1, 0), (0, 3), (0, -1)):
        with pytest.raises(_native.NativeError):
            ctx.a2c_codon_detail(SLOT, g, frame, 1)
    # a load that failed leaves the slot without one
    with pytest.raises(_native.NativeError):
        ctx.a2c_load_rows(SLOT, ['AXA'], [0], [1], [0, 1], a2c._CODON_CHARS)
    with pytest.raises(_native.NativeError):
        ctx.a2c_codon_detail(SLOT, 0, 0, 1)


# ---------------------------------------------------------------------------
# 2. the file against the oracle
# ---------------------------------------------------------------------------
def _remap(case):
    with gzip.open(os.path.join(E2E_DIR, case, 'remap.csv.gz'), 'rt') as f:
        return f.read()


def _rows(text):
    return list(csv.reader(io.StringIO(text)))


def _shift(text, column):
    """CSV text with 1 added to an integer column."""
    rows = _rows(text)
    k = rows[0].index(column)
    out = io.StringIO()
    csv.writer(out, lineterminator='\n').writerows(
        [rows[0]] + [r[:k] + [int(r[k]) + 1] + r[k + 1:] for r in rows[1:]])
    return out.getvalue()


def _sam2aln(case):
    """(aligned.csv, clipping.csv, conseq_ins.csv) texts of this build's
    sam2aln.  The goldens' regions all sit in reading frame 0, so SHIFTED is
    syn_pol_indel's files with every offset, clipped position and insertion
    position one further right, as tests/test_gpu_nuc_detail.py builds it:
    its regions read in frame 2."""
    if case == SHIFTED:
        aligned, clipping, conseq_ins = _sam2aln('syn_pol_indel')
        return _shift(aligned, 'offset'), _shift(clipping, 'pos'), _shift(conseq_ins, 'pos')
    if case not in _BUILT:
        outs = [io.StringIO() for _ in range(3)]
        s2a.sam2aln(io.StringIO(_remap(case)), outs[0], clipping_csv=outs[1], conseq_ins_csv=outs[2])
        _BUILT[case] = tuple(o.getvalue() for o in outs)
    return _BUILT[case]


def _oracle_inputs(case):
    """(clipping.csv, conseq_ins.csv) as the oracles give them."""
    if case == SHIFTED:
        clipping, conseq_ins = _oracle_inputs('syn_pol_indel')
        return _shift(clipping, 'pos'), _shift(conseq_ins, 'pos')
    remap = _remap(case)
    return clip_oracle.clipping(remap)[0], ins_oracle.conseq_ins(remap)


def _expected(case):
    """(rows, frames) amino_detail.csv must hold, built once per case."""
    if case not in _EXPECTED:
        clipping, conseq_ins = _oracle_inputs(case)
        _EXPECTED[case] = ado.expected_rows(_sam2aln(case)[0], clip_oracle.as_dict(clipping),
                                            ins_oracle.totals(conseq_ins))
    return _EXPECTED[case]


def _run(aligned_handle, clipping=None, conseq_ins=None, detail=True, nuc_detail=False, **kw):
    outs = {k: io.StringIO() for k in PLAIN + ('detail', 'nuc_detail')}
    if detail:
        kw['amino_detail_csv'] = outs['detail']
    if nuc_detail:
        kw['nuc_detail_csv'] = outs['nuc_detail']
    if clipping is not None:
        kw['clipping_csv'] = io.StringIO(clipping)
    if conseq_ins is not None:
        kw['conseq_ins_csv'] = io.StringIO(conseq_ins)
    a2c.aln2counts(aligned_handle, outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'], **kw)
    return {k: v.getvalue() for k, v in outs.items()}


@pytest.mark.parametrize('case', CASES)
def test_amino_detail_matches_the_oracle(case):
    aligned, clipping, conseq_ins = _sam2aln(case)
    assert (clipping, conseq_ins) == _oracle_inputs(case)
    want, frames = _expected(case)
    # what the inputs must hold, by the oracle alone, for the comparison to mean something
    assert sum(int(r[PARTIAL]) > 0 for r in want) > 300
    if case == 'syn_unpaired300':
        assert not any(int(r[X]) for r in want)
    else:
        assert sum(int(r[X]) > 0 for r in want) > 800
    if case == 'c1_example':
        assert not any(int(r[DEL]) for r in want)
    else:
        assert sum(int(r[DEL]) > 0 for r in want) >= 2
    if case == SHIFTED:
        assert set(frames) != {0}
        assert any(f != 0 and int(r[INS]) > 0 for r, f in zip(want, frames))
        assert any(f != 0 and int(r[CLIP]) > 0 for r, f in zip(want, frames))
    got = _run(io.StringIO(aligned), clipping, conseq_ins)
    rows = _rows(got['detail'])
    assert rows[0] == ado.HEADER
    assert rows[1:] == want
    # one row per row of amino.csv, the first 26 fields the same; coverage is the sum
    assert [r[:26] for r in rows] == _rows(got['amino'])
    assert all(int(r[COVERAGE]) == sum(int(x) for x in r[5:29]) for r in rows[1:])
    assert got['detail'].count(os.linesep) == len(rows) == got['amino'].count(os.linesep)
    # every other output is byte-equal with and without the new argument
    plain = _run(io.StringIO(aligned), clipping, conseq_ins, detail=False)
    assert all(got[k] == plain[k] for k in PLAIN) and plain['detail'] == ''


@pytest.mark.parametrize('case', ['syn_pol_indel', SHIFTED])
def test_without_the_inputs_the_columns_are_empty(case):
    aligned, clipping, conseq_ins = _sam2aln(case)
    want, _ = _expected(case)
    for clip_text, ins_text in ((None, None), (clipping, None), (None, conseq_ins)):
        rows = _rows(_run(io.StringIO(aligned), clip_text, ins_text)['detail'])
        assert rows[0] == ado.HEADER
        assert rows[1:] == [r[:INS] + [r[INS] if ins_text else '', r[CLIP] if clip_text else '', r[COVERAGE]]
                            for r in want]


@pytest.mark.parametrize('case', ['syn_pol_indel', SHIFTED])
def test_both_detail_files_in_one_call(case):
    """ins is the sum, clip the maximum of the codon's three nuc_detail.csv
    rows; nuc_detail.csv is what it is without amino_detail_csv."""
    aligned, clipping, conseq_ins = _sam2aln(case)
    got = _run(io.StringIO(aligned), clipping, conseq_ins, nuc_detail=True)
    alone = _run(io.StringIO(aligned), clipping, conseq_ins, detail=False, nuc_detail=True)
    assert got['nuc_detail'] == alone['nuc_detail']
    assert _rows(got['detail'])[1:] == _expected(case)[0]
    nuc = _rows(got['nuc_detail'])
    assert nuc[0][11] == 'clip' and nuc[0][13] == 'ins'
    by_codon = {}
    for r in nuc[1:]:
        by_codon.setdefault((r[0], r[1], r[2], (int(r[4]) + 2) // 3), []).append(r)
    checked = 0
    for r in _rows(got['detail'])[1:]:
        three = by_codon[r[0], r[1], r[2], int(r[4])]
        assert len(three) == 3
        assert int(r[INS]) == sum(int(n[13]) for n in three)
        assert int(r[CLIP]) == max(int(n[11]) for n in three)
        checked += int(r[INS]) > 0 or int(r[CLIP]) > 0
    assert checked > 10


def test_two_cutoffs_share_clip_and_have_their_own_classes():
    aligned, clipping = io.StringIO(), io.StringIO()
    s2a.sam2aln(io.StringIO(_remap('syn_pol_indel')), aligned, q_cutoffs=[10, 20], clipping_csv=clipping)
    rows = _rows(_run(io.StringIO(aligned.getvalue()), clipping.getvalue())['detail'])[1:]
    assert rows == [r[:INS] + [''] + r[CLIP:] for r in
                    ado.expected_rows(aligned.getvalue(), clip_oracle.as_dict(clipping.getvalue()))[0]]
    by_cut = {}
    for r in rows:
        if r[3] != '':
            by_cut.setdefault(r[2], {})[r[0], r[1], r[3]] = r
    assert sorted(by_cut) == ['10', '20']
    shared = set(by_cut['10']) & set(by_cut['20'])
    assert len(shared) > 100
    assert all(by_cut['10'][k][CLIP] == by_cut['20'][k][CLIP] for k in shared)
    assert any(int(by_cut['10'][k][CLIP]) > 0 for k in shared)
    assert any(by_cut['10'][k][X] != by_cut['20'][k][X] for k in shared)


def test_resident_and_file_routes_agree(tmp_path, monkeypatch):
    """aln2counts counting sam2aln's resident rows and aln2counts parsing
    aligned.csv write the same amino_detail.csv."""
    remap = tmp_path / 'remap.csv'
    remap.write_text(_remap('syn_pol_indel'))
    with open(remap) as rc, open(tmp_path / 'aligned.csv', 'w') as al, \
            open(tmp_path / 'clipping.csv', 'w') as cl, open(tmp_path / 'conseq_ins.csv', 'w') as ci:
        s2a.sam2aln(rc, al, clipping_csv=cl, conseq_ins_csv=ci)
    clipping = (tmp_path / 'clipping.csv').read_text()
    conseq_ins = (tmp_path / 'conseq_ins.csv').read_text()
    with open(tmp_path / 'aligned.csv') as al:
        dev = _run(al, clipping, conseq_ins)
    assert session.stats['aln2counts_source'] == 'device'
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    with open(tmp_path / 'aligned.csv') as al:
        file = _run(al, clipping, conseq_ins)
    assert session.stats['aln2counts_source'] == 'csv'
    assert dev == file
    assert _rows(dev['detail'])[1:] == _expected('syn_pol_indel')[0]


def test_sequence_report_after_read():
    """write_amino_detail on a SequenceReport that read() rows itself."""
    aligned = _sam2aln('syn_pol_indel')[0]
    report = a2c.SequenceReport(a2c.InsertionWriter(io.StringIO()), a2c.project_config.ProjectConfig.loadDefault(),
                                a2c.CONSEQ_MIXTURE_CUTOFFS)
    out = io.StringIO()
    report.write_amino_detail_header(out)
    for group in ado.groups(aligned):
        report.read(group)
        report.write_amino_detail(out)
    want = [r[:INS] + ['', '', r[COVERAGE]] for r in _expected('syn_pol_indel')[0]]
    assert _rows(out.getvalue()) == [ado.HEADER] + want


def test_a_seed_without_coordinate_regions_writes_no_rows(tmp_path):
    """S4-seed of the edge cases' project file has no coordinate region:
    amino.csv holds its header alone, and so does amino_detail.csv."""
    with open(os.path.join(REPO, 'tests', 'golden', 'aln2counts_edge.json')) as f:
        edge = json.load(f)
    config = tmp_path / 'projects.json'
    config.write_text(json.dumps(edge['config']))
    text = 'refname,qcut,rank,count,offset,seq\nS4-seed,15,0,3,0,ANA---ACGnnnTT-\n'
    got = _run(io.StringIO(text), json=str(config))
    assert _rows(got['detail']) == [ado.HEADER] and _rows(got['amino']) == [ado.HEADER[:26]]
    assert len(_rows(got['nuc'])) > 10


def test_cli_flag_writes_the_same_file(tmp_path):
    aligned, clipping, conseq_ins = _sam2aln('syn_pol_indel')
    for name, text in (('aligned', aligned), ('clipping', clipping), ('conseq_ins', conseq_ins)):
        (tmp_path / (name + '.csv')).write_text(text)
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, 'micall-lite_amd'))
    subprocess.run([sys.executable, '-m', 'micall_amd.aln2counts', 'aligned.csv', 'nuc.csv', 'amino.csv',
                    'coord_ins.csv', 'conseq.csv', '--clipping_csv', 'clipping.csv', '--conseq_ins_csv',
                    'conseq_ins.csv', '--amino_detail_csv', 'amino_detail.csv'],
                   cwd=str(tmp_path), env=env, check=True, timeout=300)
    got = _run(io.StringIO(aligned), clipping, conseq_ins)
    with open(tmp_path / 'amino_detail.csv', newline='') as f:
        assert f.read() == got['detail']
    with open(tmp_path / 'amino.csv', newline='') as f:
        assert f.read() == got['amino']

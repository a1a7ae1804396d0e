"""aln2counts' nuc_detail.csv (SequenceReport.write_nuc_detail): nuc.csv's
rows with the N, deletion, soft-clip and coverage counts of each position.
aligned.csv and clipping.csv come from this build's sam2aln on the golden
remap.csv; the expected rows are built here from the oracle's Report
(oracle/og_aln2counts.py) after read() -- walked as its write_nuc_counts
walks, N / del from the position's tally -- and the clip column from
tests/clip_oracle.py at consensus position query.nuc.pos - reading frame."""
import csv
import gzip
import io
import itertools
import os

import pytest

import clip_oracle
import og_aln2counts as og
from micall_amd import aln2counts as a2c
from micall_amd import sam2aln as s2a
from micall_amd import session

pytestmark = pytest.mark.gpu

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')
SHIFTED = 'syn_pol_indel+1'
CASES = ['c1_example', 'syn_hiv3', 'syn_pol_indel', SHIFTED]
HEADER = ['seed', 'region', 'q-cutoff', 'query.nuc.pos', 'refseq.nuc.pos', 'A', 'C', 'G', 'T',
          'N', 'del', 'clip', 'coverage']
PLAIN = ('nuc', 'amino', 'coord_ins', 'conseq')
_BUILT = {}
_EXPECTED = {}


def _remap(case):
    with gzip.open(os.path.join(E2E_DIR, case, 'remap.csv.gz'), 'rt') as f:
        return f.read()


def _shift(text, column):
    """CSV text with 1 added to an integer column."""
    rows = _rows(text)
    k = rows[0].index(column)
    out = io.StringIO()
    csv.writer(out, lineterminator='\n').writerows(
        [rows[0]] + [r[:k] + [int(r[k]) + 1] + r[k + 1:] for r in rows[1:]])
    return out.getvalue()


def _sam2aln(case):
    """(aligned.csv, clipping.csv) texts of this build's sam2aln.  The
    goldens' regions all sit in reading frame 0, so SHIFTED is a directed
    pair of files: syn_pol_indel's with every offset and every clipped
    position one further right, as if the sample's consensus began one base
    earlier -- its regions then read in frame 2."""
    if case == SHIFTED:
        aligned, clipping = _sam2aln('syn_pol_indel')
        return _shift(aligned, 'offset'), _shift(clipping, 'pos')
    if case not in _BUILT:
        aligned, clipping = io.StringIO(), io.StringIO()
        s2a.sam2aln(io.StringIO(_remap(case)), aligned, clipping_csv=clipping)
        _BUILT[case] = aligned.getvalue(), clipping.getvalue()
    return _BUILT[case]


def _oracle_clipping(case):
    """clipping.csv as tests/clip_oracle.py gives it for the case."""
    if case == SHIFTED:
        return _shift(_oracle_clipping('syn_pol_indel'), 'pos')
    return clip_oracle.clipping(_remap(case))[0]


def _expected(case, with_clip=True):
    """The rows nuc_detail.csv must hold, and the reading frame of each
    (built once per case)."""
    if case not in _EXPECTED:
        _EXPECTED[case] = _build_expected(case)
    rows, frames = _EXPECTED[case]
    if not with_clip:
        rows = [r[:11] + ['', r[12]] for r in rows]
    return rows, frames


def _build_expected(case):
    aligned, _ = _sam2aln(case)
    clips = clip_oracle.as_dict(_oracle_clipping(case))
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    rows, frames = [], []
    # Report.read translates every codon of every row anew, most of its time
    # on c1_example: the same answers from a table while this runs
    translate, seen = og.translate, {}

    def memo(*args):
        if args not in seen:
            seen[args] = translate(*args)
        return seen[args]

    def emit(region, t, pos, f):
        for i, nt in enumerate(t.nucleotides):
            qpos = '' if t.consensus_index is None else i + 3 * t.consensus_index + 1
            rpos = '' if pos is None else i + 3 * pos - 2
            six = [nt.counts[b] for b in 'ACGTN-']
            clip = 0 if qpos == '' else clips.get((rep.seed, qpos - f), 0)
            rows.append([str(x) for x in [rep.seed, region, rep.qcut, qpos, rpos] + six +
                         [clip, sum(six)]])
            frames.append(f)
    og.translate = memo
    try:
        for _key, group in itertools.groupby(csv.DictReader(io.StringIO(aligned)),
                                             lambda r: (r['refname'], r['qcut'])):
            rep.read(group)
            if not rep.coordinate_refs:
                for t in rep.seed_aminos[0]:
                    emit(rep.seed, t, None, 0)
            else:
                for region, mapped in rep.reports.items():
                    for t, pos in mapped:
                        emit(region, t, pos, rep.reading_frames.get(region, 0))
    finally:
        og.translate = translate
    return rows, frames


def _run(aligned_handle, clipping_text, detail=True):
    outs = {k: io.StringIO() for k in PLAIN + ('detail',)}
    kw = {}
    if detail:
        kw['nuc_detail_csv'] = outs['detail']
        if clipping_text is not None:
            kw['clipping_csv'] = io.StringIO(clipping_text)
    a2c.aln2counts(aligned_handle, outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'], **kw)
    return {k: v.getvalue() for k, v in outs.items()}


def _rows(text):
    return list(csv.reader(io.StringIO(text)))


@pytest.mark.parametrize('case', CASES)
def test_nuc_detail_matches_the_oracle(case):
    aligned, clipping = _sam2aln(case)
    assert clipping == _oracle_clipping(case)
    got = _run(io.StringIO(aligned), clipping)
    want, _ = _expected(case)
    rows = _rows(got['detail'])
    assert rows[0] == HEADER
    assert rows[1:] == want
    assert len(want) > 100
    # one row per row of nuc.csv, the first nine fields the same
    assert [r[:9] for r in rows] == _rows(got['nuc'])
    assert all(int(r[12]) == sum(int(x) for x in r[5:11]) for r in rows[1:])
    # nothing else changes
    plain = _run(io.StringIO(aligned), None, detail=False)
    assert all(got[k] == plain[k] for k in PLAIN)
    assert plain['detail'] == ''


@pytest.mark.parametrize('case', CASES)
def test_no_clipping_csv_leaves_the_column_empty(case):
    aligned, _ = _sam2aln(case)
    rows = _rows(_run(io.StringIO(aligned), None)['detail'])
    assert rows[1:] == _expected(case, with_clip=False)[0]
    assert all(r[11] == '' for r in rows[1:]) and len(rows) > 100


def test_the_frame_shift_is_exercised():
    """Some expected row has clip > 0 under a region whose reading frame is
    not 0 (else the lookup at query.nuc.pos - frame is not tested), and a
    lookup without the frame would give other counts."""
    rows, frames = _expected(SHIFTED)
    assert sum(1 for r, f in zip(rows, frames) if f != 0 and int(r[11]) > 0) > 100
    clips = clip_oracle.as_dict(_oracle_clipping(SHIFTED))
    assert any(int(r[11]) != clips.get((r[0], int(r[3])), 0) for r in rows if r[3] != '')


def test_every_cutoff_of_a_seed_gets_the_same_clip():
    aligned, clipping = io.StringIO(), io.StringIO()
    s2a.sam2aln(io.StringIO(_remap('syn_pol_indel')), aligned, q_cutoffs=[10, 15], clipping_csv=clipping)
    rows = _rows(_run(io.StringIO(aligned.getvalue()), clipping.getvalue())['detail'])[1:]
    by_cut = {}
    for r in rows:
        by_cut.setdefault(r[2], []).append((r[0], r[1], r[3], r[11]))
    assert sorted(by_cut) == ['10', '15']
    clip = [{(seed, region, q): c for seed, region, q, c in v if q != ''} for v in by_cut.values()]
    shared = set(clip[0]) & set(clip[1])
    assert len(shared) > 100 and all(clip[0][k] == clip[1][k] for k in shared)
    assert any(int(clip[0][k]) > 0 for k in shared)


def test_resident_and_file_routes_agree(tmp_path, monkeypatch):
    """aln2counts counting sam2aln's resident rows and aln2counts parsing
    aligned.csv write the same nuc_detail.csv."""
    remap = tmp_path / 'remap.csv'
    remap.write_text(_remap('c1_example'))
    with open(remap) as rc, open(tmp_path / 'aligned.csv', 'w') as al, \
            open(tmp_path / 'clipping.csv', 'w') as cl:
        s2a.sam2aln(rc, al, clipping_csv=cl)
    clipping = (tmp_path / 'clipping.csv').read_text()
    with open(tmp_path / 'aligned.csv') as al:
        dev = _run(al, clipping)
    assert session.stats['aln2counts_source'] == 'device'
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    with open(tmp_path / 'aligned.csv') as al:
        file = _run(al, clipping)
    assert session.stats['aln2counts_source'] == 'csv'
    assert dev == file
    assert _rows(dev['detail'])[1:] == _expected('c1_example')[0]

"""The ins column of aln2counts' nuc_detail.csv: with conseq_ins_csv (sam2aln's
conseq_ins.csv) every row ends with the units that carry an insertion after
the row's consensus position, at the row's q-cutoff.  The expected file is
the call without conseq_ins_csv with the column appended from
tests/ins_oracle.py's counts at consensus position query.nuc.pos - reading
frame; the frame comes from the oracle's Report (oracle/og_aln2counts.py)."""
import csv
import gzip
import io
import itertools
import os

import pytest

import ins_oracle
import og_aln2counts as og
from micall_amd import aln2counts as a2c
from micall_amd import sam2aln as s2a
from micall_amd import session

pytestmark = pytest.mark.gpu

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')
CASES = ['syn_pol', 'syn_pol_indel', 'c1_example']
PLAIN = ('nuc', 'amino', 'coord_ins', 'conseq')
_BUILT = {}


def _remap(case):
    with gzip.open(os.path.join(E2E_DIR, case, 'remap.csv.gz'), 'rt') as f:
        return f.read()


def _sam2aln(case):
    """(aligned.csv, clipping.csv, conseq_ins.csv) texts of this build's
    sam2aln on the golden remap.csv, once per case."""
    if case not in _BUILT:
        outs = [io.StringIO() for _ in range(3)]
        s2a.sam2aln(io.StringIO(_remap(case)), outs[0], clipping_csv=outs[1], conseq_ins_csv=outs[2])
        _BUILT[case] = tuple(o.getvalue() for o in outs)
    return _BUILT[case]


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


def _run(aligned_handle, clipping, conseq_ins):
    outs = {k: io.StringIO() for k in PLAIN + ('detail',)}
    kw = dict(nuc_detail_csv=outs['detail'], clipping_csv=io.StringIO(clipping))
    if conseq_ins is not None:
        kw['conseq_ins_csv'] = io.StringIO(conseq_ins)
    a2c.aln2counts(aligned_handle, outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'], **kw)
    return {k: v.getvalue() for k, v in outs.items()}


def _rows(text):
    return list(csv.reader(io.StringIO(text)))


@pytest.mark.parametrize('case', CASES)
def test_ins_column_is_the_oracles(case):
    aligned, clipping, conseq_ins = _sam2aln(case)
    want_ins = ins_oracle.conseq_ins(_remap(case))
    assert conseq_ins == want_ins
    today = _run(io.StringIO(aligned), clipping, None)
    got = _run(io.StringIO(aligned), clipping, conseq_ins)
    # every other output is byte-equal in both calls
    assert all(got[k] == today[k] for k in PLAIN)
    totals = ins_oracle.totals(want_ins)
    frames = _frames(aligned)
    rows = _rows(today['detail'])
    want = [rows[0] + ['ins']]
    for r in rows[1:]:
        seed, region, qcut, query = r[0], r[1], int(r[2]), r[3]
        n = 0 if query == '' else totals.get((seed, qcut, int(query) - frames[seed, region]), 0)
        want.append(r + [str(n)])
    assert _rows(got['detail']) == want
    ins = [int(r[-1]) for r in want[1:]]
    assert any(n > 0 for n in ins)
    if case == 'syn_pol':
        assert max(ins) >= 150


def test_without_conseq_ins_nothing_changes():
    """The header and rows have no ins column, as before this option."""
    aligned, clipping, _ = _sam2aln('syn_pol')
    rows = _rows(_run(io.StringIO(aligned), clipping, None)['detail'])
    assert rows[0][-1] == 'coverage' and all(len(r) == 13 for r in rows) and len(rows) > 100


def test_resident_and_file_routes_agree(tmp_path, monkeypatch):
    """aln2counts counting sam2aln's resident rows and aln2counts parsing
    aligned.csv write the same nuc_detail.csv with the ins column."""
    remap = tmp_path / 'remap.csv'
    remap.write_text(_remap('syn_pol_indel'))
    with open(remap) as rc, open(tmp_path / 'aligned.csv', 'w') as al, \
            open(tmp_path / 'clipping.csv', 'w') as cl, open(tmp_path / 'conseq_ins.csv', 'w') as ci:
        s2a.sam2aln(rc, al, clipping_csv=cl, conseq_ins_csv=ci)
    clipping = (tmp_path / 'clipping.csv').read_text()
    conseq_ins = (tmp_path / 'conseq_ins.csv').read_text()
    assert conseq_ins == _sam2aln('syn_pol_indel')[2]
    with open(tmp_path / 'aligned.csv') as al:
        dev = _run(al, clipping, conseq_ins)
    assert session.stats['aln2counts_source'] == 'device'
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    with open(tmp_path / 'aligned.csv') as al:
        file = _run(al, clipping, conseq_ins)
    assert session.stats['aln2counts_source'] == 'csv'
    assert dev == file
    assert _rows(dev['detail'])[0][-1] == 'ins' and any(int(r[-1]) > 0 for r in _rows(dev['detail'])[1:])

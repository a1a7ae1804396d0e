"""tests/strand_oracle.py, the specification of sam2aln's strand.csv, against
counts worked out by hand (tests/strand_cases.py) and against the reference:
for every (refname, qcut, pos) and base, fwd + rev - both must be the count of
the golden aligned.csv rows that hold the base there.  The device tests
(tests/test_gpu_strand.py) compare with this oracle byte for byte."""
import csv
import gzip
import io
import os

import pytest

import og_sam2aln
import strand_cases as cases
import strand_oracle as oracle

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
HEAD = ','.join(cases.HEADER) + '\n'
_SEEN = {}


def _golden_text(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.gz'), 'rt') as f:
        return f.read()


def _golden(case):
    """The oracle's counts of a golden remap.csv at cutoff 15, computed once."""
    if case not in _SEEN:
        _SEEN[case] = oracle.count(_golden_text(case, 'remap.csv'))
    return _SEEN[case]


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_hand_written_case(name):
    rows, cuts, want = cases.CASES[name]
    text = cases.text(rows)
    assert oracle.count(text, cuts) == want
    assert oracle.strand(text, cuts) == cases.expected_text(want, cuts)
    if name in cases.HEADER_ALONE:
        assert oracle.strand(text, cuts) == HEAD
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = list(cuts)
    try:
        aligned, _, failed = og_sam2aln.sam2aln(text)
    finally:
        og_sam2aln.Q_CUTOFFS = saved
    causes = [f['cause'] for f in csv.DictReader(io.StringIO(failed))]
    assert causes == ([cases.FAILED_CAUSE[name]] if name in cases.FAILED_CAUSE else [])
    # the identity with aligned.csv holds wherever the forward read starts
    if name != 'forward_never_starts':
        assert oracle.called(want) == oracle.aligned_calls(aligned)


def test_cases_cover_every_column_and_the_order():
    rows, want = cases.combined()
    assert oracle.count(cases.text(rows)) == want
    sums = [sum(v[k] for v in want.values()) for k in range(15)]
    assert all(sums), sums
    assert og_sam2aln.Q_CUTOFFS == [15]           # restored after every count
    text = oracle.strand(cases.text(cases.CASES['two_refs'][0]))
    assert [line.split(',')[0] for line in text.splitlines()[1:]] == ['alpha'] * 4 + ['zeta'] * 12
    text = oracle.strand(cases.text(cases.CASES['unsorted_cutoffs'][0]), [30, 10])
    assert [line.split(',')[1] for line in text.splitlines()[1:]] == ['30'] * 9 + ['10'] * 10
    assert oracle.strand(cases.text([])) == HEAD
    assert oracle.rows(text) == oracle.count(cases.text(cases.CASES['unsorted_cutoffs'][0]), [30, 10])


@pytest.mark.parametrize('case', E2E)
def test_identity_with_the_golden_aligned_csv(case):
    """fwd + rev - both of every base is the count of the reference's own
    aligned.csv rows that hold it there, deletions included."""
    counts = _golden(case)
    assert oracle.called(counts) == oracle.aligned_calls(_golden_text(case, 'aligned.csv'))
    assert all(v[3 * k + 2] <= min(v[3 * k], v[3 * k + 1]) for v in counts.values() for k in range(5))


def test_identity_at_several_cutoffs():
    cuts = [0, 10, 15, 30]
    text = _golden_text('syn_pol_indel', 'remap.csv')
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = cuts
    try:
        aligned = og_sam2aln.sam2aln(text)[0]
    finally:
        og_sam2aln.Q_CUTOFFS = saved
    counts = oracle.count(text, cuts)
    assert og_sam2aln.Q_CUTOFFS == saved
    assert {q for _, q, _ in counts} == set(cuts)
    assert oracle.called(counts) == oracle.aligned_calls(aligned)
    assert {k: v for k, v in counts.items() if k[1] == 15} == _golden('syn_pol_indel')


def test_golden_figures():
    """The figures a plain dict-per-position prototype gave for the goldens."""
    c1 = _golden('c1_example')
    assert len(c1) == 3010
    assert [sum(v[k] for v in c1.values()) for k in range(3)] == [891381, 898475, 571824]
    assert [sum(v[k] for v in _golden('micro_2060A-V3LOOP').values()) for k in range(3)] == [300, 250, 30]
    assert [sum(v[k] for v in _golden('micro_2070A-PR').values()) for k in (12, 13, 14)] == [51, 51, 51]
    unpaired = _golden('syn_unpaired300')
    assert unpaired and all(v[3 * k + 1] == 0 and v[3 * k + 2] == 0 for v in unpaired.values() for k in range(5))
    for case in ('syn_noseed', 'micro_2030A-V3LOOP', 'micro_2050A-V3LOOP'):
        assert oracle.text(_golden(case)) == HEAD

"""tests/concordance_oracle.py, the specification of sam2aln's concordance.csv
and cycle_concordance.csv, against counts worked out by hand
(tests/concordance_cases.py), the totals of the golden remap.csv files found
with an independent script, and the identities that tie the two files
together.  The device tests (tests/test_gpu_concordance.py) compare with this
oracle byte for byte."""
import csv
import gzip
import io
import os

import pytest

import concordance_cases as cases
import concordance_oracle as oracle
import og_sam2aln

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
HEADS = ('refname,pos,overlap,mismatch,indel,nocall,unresolved\n', 'read,by,value,compared,mismatch\n')
_SEEN = {}


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_hand_written_case(name):
    rows, want_p, want_r = cases.CASES[name]
    text = cases.text(rows)
    assert oracle.concordance(text) == cases.expected_texts(want_p, want_r)
    if name in cases.NOT_COUNTED:
        assert oracle.concordance(text) == HEADS
    # what failed.csv says of the unit: only manyNs units are counted
    failed = list(csv.DictReader(io.StringIO(og_sam2aln.sam2aln(text)[2])))
    assert [f['cause'] for f in failed] == ([cases.FAILED_CAUSE[name]] if name in cases.FAILED_CAUSE else [])


def test_hand_written_cases_cover_every_class():
    rows, want_p, want_r = cases.combined()
    assert oracle.concordance(cases.text(rows)) == cases.expected_texts(want_p, want_r)
    sums = [sum(v[k] for v in want_p.values()) for k in range(5)]
    assert all(sums), sums                       # overlap, mismatch, indel, nocall, unresolved
    assert max(v[0] for v in want_p.values()) >= 10
    assert len({name for name, _ in want_p}) == 3
    assert max(value for _, by, value in want_r if by == 'cycle') == 2000


def test_text_format():
    """Headers, '\\n' line ends, names quoted as csv quotes them, references
    as Python sorts str, positions and values numerically, cycle before
    quality."""
    rows = (cases._clean('a', 9, 3, 10, 2, ref='b,1')[0] + cases._clean('b', 100, 1, 100, 1, ref='B')[0])
    got = oracle.concordance(cases.text(rows))
    assert got[0] == HEADS[0] + 'B,100,1,0,0,0,0\n"b,1",10,1,0,0,0,0\n"b,1",11,1,0,0,0,0\n'
    assert got[1] == HEADS[1] + ('1,cycle,1,1,0\n1,cycle,2,1,0\n1,cycle,3,1,0\n1,quality,40,3,0\n'
                                 '2,cycle,1,2,0\n2,cycle,2,1,0\n2,quality,40,3,0\n')
    assert oracle.concordance(','.join(cases.HEADER) + '\n') == HEADS


def _golden(case):
    if case not in _SEEN:
        with gzip.open(os.path.join(E2E_DIR, case, 'remap.csv.gz'), 'rt') as f:
            text = f.read()
        _SEEN[case] = oracle.count(text) + (text,)
    return _SEEN[case]


def _sums(case):
    positions = _golden(case)[0]
    return [sum(v[k] for v in positions.values()) for k in range(5)]


def test_golden_totals():
    """The figures an independent script gave for the goldens."""
    overlap, mismatch, indel, nocall, unresolved = _sums('c1_example')
    assert (overlap, len(_golden('c1_example')[0])) == (1443257, 2812)
    assert (mismatch, indel, unresolved) == (10094, 22, 537)
    assert _sums('syn_pol_indel')[2] == 50
    for case in ('syn_noseed', 'micro_2030A-V3LOOP', 'syn_unpaired300'):
        assert oracle.concordance(_golden(case)[2]) == HEADS
    # no golden has a nocall: the hand-written cases must cover it, and do
    assert all(_sums(case)[3] == 0 for case in E2E)
    assert sum(v[3] for v in cases.combined()[1].values()) > 0


def test_goldens_exercise_the_pass():
    """What the device tests compare with is more than headers on most goldens."""
    assert oracle.position_text(_golden('c1_example')[0]).count('\n') == 2813
    assert sum(1 for case in E2E if oracle.concordance(_golden(case)[2]) != HEADS) >= 5


@pytest.mark.parametrize('case', E2E)
def test_identities(case):
    positions, reads, text = _golden(case)

    def total(read, by, k):
        return sum(v[k] for (r, b, _), v in reads.items() if r == read and b == by)

    assert total(1, 'cycle', 0) == total(2, 'cycle', 0)
    for read in (1, 2):
        assert total(read, 'cycle', 0) == total(read, 'quality', 0)
        assert total(read, 'cycle', 1) == total(read, 'quality', 1)
    by_position = sum(v[1] for v in positions.values())
    assert by_position <= total(1, 'cycle', 1)
    literal_dash = any('-' in r['seq'] for r in csv.DictReader(io.StringIO(text)))
    if not literal_dash:
        assert by_position == total(1, 'cycle', 1)
    assert all(v[0] >= v[1] + v[2] + v[3] and v[4] <= v[1] + v[2] + v[3] for v in positions.values())


def test_literal_dash_breaks_the_equality():
    rows, want_p, want_r = cases.CASES['literal_dash']
    assert sum(v[1] for v in want_p.values()) == 0 and want_r[1, 'cycle', 4] == [1, 1]

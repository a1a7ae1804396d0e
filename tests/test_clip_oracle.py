"""tests/clip_oracle.py, the specification of sam2aln's clipping.csv, against
clipping.csv texts worked out by hand (tests/clip_cases.py), and the
conditions on the golden remap.csv files that keep the device tests
(tests/test_gpu_clipping.py) from passing vacuously: enough rows, enough
pairs that lose a clipped position to the mate, pairs whose mates clip a
common position."""
import csv
import gzip
import io
import os

import pytest

import clip_cases
import clip_oracle
import og_sam2aln

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')


@pytest.mark.parametrize('name', sorted(clip_cases.CASES))
def test_hand_written_case(name):
    rows, want = clip_cases.CASES[name]
    got, tallies = clip_oracle.clipping(clip_cases.text(rows))
    assert got == clip_cases.expected_text(want)
    assert tallies['contributing'] == (1 if want else 0) * tallies['units']
    # what failed.csv says of the unit: only manyNs units are counted
    failed = list(csv.DictReader(io.StringIO(og_sam2aln.sam2aln(clip_cases.text(rows))[2])))
    assert [f['cause'] for f in failed] == ([clip_cases.FAILED_CAUSE[name]]
                                            if name in clip_cases.FAILED_CAUSE else [])
    assert tallies['units'] == (0 if name in ('unmatched', 'bad_cigar', 'two_refs_pair')
                                else len({r[0] for r in rows}))


def test_combined_cases_add_up():
    rows, want = clip_cases.combined()
    got, tallies = clip_oracle.clipping(clip_cases.text(rows))
    assert got == clip_cases.expected_text(want)
    assert max(want.values()) >= 3           # positions several units clip
    assert tallies['common'] == 2 and tallies['lost_to_mate'] == 2


def test_text_format():
    """Header, '\\n' line ends, names quoted as csv quotes them, references
    as Python sorts str and positions numerically (-3 before 1 before 10)."""
    rows = [clip_cases.row('a', 0, 'b,1', 2, '5S4M'), clip_cases.row('b', 0, 'B', 10, '1S4M'),
            clip_cases.row('c', 0, 'b,1', 10, '4M1S')]
    got, _ = clip_oracle.clipping(clip_cases.text(rows))
    assert got == ('refname,pos,count\nB,9,1\n"b,1",-3,1\n"b,1",-2,1\n"b,1",-1,1\n"b,1",0,1\n'
                   '"b,1",1,1\n"b,1",14,1\n')
    assert clip_oracle.clipping('qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n')[0] == \
        'refname,pos,count\n'


# what the goldens must hold for the device tests to mean something (the
# figures seen with this oracle: 2880, 4204, 233, 8, 14)
GOLDEN_FLOORS = [('c1_example', 'rows', 2000), ('c1_example', 'contributing', 4000),
                 ('c1_example', 'lost_to_mate', 200), ('syn_pol_indel', 'common', 5),
                 ('syn_maxremaps', 'common', 5)]
_SEEN = {}


def _golden(case):
    if case not in _SEEN:
        with gzip.open(os.path.join(E2E_DIR, case, 'remap.csv.gz'), 'rt') as f:
            text, tallies = clip_oracle.clipping(f.read())
        _SEEN[case] = dict(tallies, rows=text.count('\n') - 1)
    return _SEEN[case]


@pytest.mark.parametrize('case,what,floor', GOLDEN_FLOORS)
def test_goldens_are_not_vacuous(case, what, floor):
    assert _golden(case)[what] >= floor, _golden(case)

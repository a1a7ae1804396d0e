"""tests/ins_oracle.py, the specification of sam2aln's conseq_ins.csv: its
merge_inserts against every call of the reference's that
tests/golden/sam2aln_golden.json records, the whole rule against rows worked
out by hand (tests/ins_cases.py), and what the golden remap.csv files hold,
so that the device tests (tests/test_gpu_conseq_ins.py) do not pass
vacuously."""
import csv
import gzip
import io
import json
import os

import pytest

import ins_cases
import ins_oracle
import og_sam2aln

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
E2E = sorted(os.listdir(E2E_DIR))
HEAD_ONLY = 'refname,qcut,pos,insert,count\n'


def _dec(x):
    """gen_golden.py's encoding of dicts (keys need not be strings) undone."""
    if isinstance(x, dict):
        return {_key(_dec(k)): _dec(v) for k, v in x['__dict__']}
    if isinstance(x, list):
        return [_dec(v) for v in x]
    return x


def _key(k):
    return tuple(k) if isinstance(k, list) else k


def _recorded():
    with open(os.path.join(HERE, 'golden', 'sam2aln_golden.json')) as f:
        calls = [_dec(c) for c in json.load(f)['cases']]
    return [c for c in calls if c['fn'] == 'merge_inserts']


def test_merge_inserts_reproduces_the_recorded_calls():
    calls = _recorded()
    assert len(calls) == 11
    assert sum(1 for c in calls if c['kwargs'].get('minimum_q_delta') == 20) == 1
    for c in calls:
        args = [None if a is None else {k: tuple(v) for k, v in a.items()} if isinstance(a, dict) else a
                for a in c['args']]
        assert ins_oracle.merge_inserts(*args, **c['kwargs']) == c['result'], c


@pytest.mark.parametrize('name', sorted(ins_cases.CASES))
def test_hand_written_case(name):
    rows, cuts, want = ins_cases.CASES[name]
    text = ins_cases.text(rows)
    assert ins_oracle.conseq_ins(text, cuts) == ins_cases.expected_text(want)
    # what failed.csv says of the case's units at the default cutoff
    failed = list(csv.DictReader(io.StringIO(og_sam2aln.sam2aln(text)[2])))
    cause = ins_cases.FAILED_CAUSE.get(name, 'manyNs' if name == 'many_ns_at_15' else None)
    assert [f['cause'] for f in failed] == ([cause] if cause else [])


def test_keys_differ_from_insert_csv():
    """insert.csv's pos is POS - 1 + the read offset: 16 after the 3-base
    clip, 13 after the deletion, where the keys are 13 and 15."""
    for name, pos in (('after_soft_clip', 16), ('after_deletion', 13)):
        rows = ins_cases.CASES[name][0]
        ins = list(csv.DictReader(io.StringIO(og_sam2aln.sam2aln(ins_cases.text(rows))[1])))
        assert [int(r['pos']) for r in ins] == [pos]
        assert ins_cases.CASES[name][2][0][2] != pos


def test_combined_cases_add_up():
    rows, want = ins_cases.combined()
    assert ins_oracle.conseq_ins(ins_cases.text(rows)) == ins_cases.expected_text(want)
    assert sum(1 for r in want if r[4] >= 2) >= 3      # rows that several cases share
    assert [r[0] for r in want] == sorted(r[0] for r in want) and len({r[0] for r in want}) == 4


def test_text_format():
    """'\\n' line ends, names quoted as csv quotes them, and the header alone
    for a text without insertions."""
    rows = ins_cases.CASES['two_refs'][0]
    assert ins_oracle.conseq_ins(ins_cases.text(rows)) == \
        'refname,qcut,pos,insert,count\nalpha,15,51,C,1\n"b,1",15,10,TT,1\nzeta,15,13,G,1\n'
    assert ins_oracle.conseq_ins(','.join(ins_cases.HEADER) + '\n') == HEAD_ONLY


def test_a_dash_is_refused_by_read_name():
    rows = [ins_cases.read('fine', 0, 'R1', 10, 'M4', ('I', 'GG'), 'M4'),
            ins_cases.read('dashed', 0, 'R1', 10, 'M4', ('I', 'G-'), 'M4')]
    with pytest.raises(ins_oracle.Refused, match='dashed'):
        ins_oracle.conseq_ins(ins_cases.text(rows))


# ---------------------------------------------------------------------------
# the goldens at cutoff 15: (rows, unit x insertion) per case with I ops
# ---------------------------------------------------------------------------
WITH_I_OPS = {'c1_example': (7, 7), 'syn_chimera': (5, 104), 'syn_hiv3': (2, 94),
              'syn_maxremaps': (34, 415), 'syn_pol': (5, 168), 'syn_pol_indel': (32, 640),
              'syn_unpaired300': (1, 60)}
_SEEN = {}


def _golden(case):
    if case not in _SEEN:
        with gzip.open(os.path.join(E2E_DIR, case, 'remap.csv.gz'), 'rt') as f:
            text = f.read()
        counts, tallies = ins_oracle.counts(text)
        _SEEN[case] = dict(tallies, rows=len(counts), text=ins_oracle.to_text(ins_oracle.ordered(counts)),
                           i_ops=any('I' in r['cigar'] for r in csv.DictReader(io.StringIO(text))))
    return _SEEN[case]


@pytest.mark.parametrize('case', E2E)
def test_goldens_hold_insertions_where_they_hold_i_ops(case):
    g = _golden(case)
    assert g['i_ops'] == (case in WITH_I_OPS)
    assert (g['text'] != HEAD_ONLY) == (case in WITH_I_OPS)
    if case in WITH_I_OPS:
        assert (g['rows'], g['insertions']) == WITH_I_OPS[case]


def test_syn_pol_indel_merges_from_both_mates():
    assert _golden('syn_pol_indel')['both'] >= 50


def test_syn_pol_has_one_dominant_insertion():
    rows = list(csv.DictReader(io.StringIO(_golden('syn_pol')['text'])))
    top = max(rows, key=lambda r: int(r['count']))
    assert int(top['count']) >= 150 and len(top['insert']) == 3

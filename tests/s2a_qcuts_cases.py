"""Shared by the multi-cutoff sam2aln tests: the cases of
tests/golden/sam2aln_qcuts.json (see tests/golden/gen_golden_qcuts.py for
its layout) and the comparison of a text with a stored output."""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
HEAD = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'

with open(os.path.join(GOLDEN, 'sam2aln_qcuts.json')) as _f:
    CASES = json.load(_f)['cases']
with open(os.path.join(GOLDEN, 'sam2aln_e2e.json')) as _f:
    E2E_JSON = json.load(_f)['cases']


def case_id(k):
    c = CASES[k]
    return '{}-{}'.format(c['name'].split(' ')[0], '_'.join(map(str, c['q_cutoffs'])))


def remap_text(case):
    if 'remap_csv' in case:
        return case['remap_csv']
    return E2E_JSON[case['e2e_json_case']]['remap_csv']


def assert_equals_golden(text, want, what):
    """want: the text itself, or {'sha256', 'bytes'} of a long one."""
    if isinstance(want, str):
        assert text == want, what
        return
    data = text.encode()
    assert len(data) == want['bytes'], what
    assert hashlib.sha256(data).hexdigest() == want['sha256'], what


def tiny_text():
    """The eight-base example: p1 fails at 15 only, p3 at every cutoff."""
    rows = []
    for name, qual in (('p1', '-----???'), ('p2', '????????'), ('p3', '!!!!!!!!')):
        for flag in (99, 147):
            rows.append('{},{},R,1,44,8M,=,1,8,ACGTACGT,{}\n'.format(name, flag, qual))
    return HEAD + ''.join(rows)

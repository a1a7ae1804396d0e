"""The oracle restatement of sam2aln (oracle/og_sam2aln.py) with a list of
q-cutoffs against the reference's own outputs for the same list
(tests/golden/sam2aln_qcuts.json, written by tests/golden/gen_golden_qcuts.py
from micall.core.sam2aln.sam2aln with SAM2ALN_Q_CUTOFFS patched): byte-equal
aligned.csv, insert.csv and failed.csv.  No device needed.  This pins the
oracle on the ground the multi-cutoff device tests compare against it on."""
import pytest

import og_sam2aln
import s2a_qcuts_cases as qc


@pytest.mark.parametrize('k', range(len(qc.CASES)), ids=qc.case_id)
def test_oracle_matches_reference_at_every_cutoff_list(k, monkeypatch):
    case = qc.CASES[k]
    monkeypatch.setattr(og_sam2aln, 'Q_CUTOFFS', list(case['q_cutoffs']))
    got = og_sam2aln.sam2aln(qc.remap_text(case))
    for name, text in zip(('aligned', 'insert', 'failed'), got):
        qc.assert_equals_golden(text, case[name], (case['name'], case['q_cutoffs'], name))


def test_golden_holds_every_list_for_every_text():
    """The file is the cross product the device tests lean on: 5 lists for
    each of the tiny example, the 13 sam2aln_e2e.json texts, two e2e cases and
    the unpaired text."""
    names = sorted({c['name'] for c in qc.CASES})
    assert len(names) == 17
    for n in names:
        lists = [c['q_cutoffs'] for c in qc.CASES if c['name'] == n]
        assert lists == [[0, 10, 15], [15, 10, 0], [15, 15], [20], [0, 93]], n

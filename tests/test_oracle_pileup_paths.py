"""The oracle pileup pinned to the reference's own counters on the directed
path cases of tests/pileup_path_cases.py (tests/golden/pileup_paths.json,
written by tests/golden/gen_pileup_paths.py from the reference's
sam_to_conseqs): same generated text (SHA-256), same counters at every
position, same reference order, same consensus, at cutoffs 0 and 20."""
import json
import os

import pytest

import oracle
import pileup_path_cases as ppc


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'pileup_paths.json')) as f:
        return {(c['name'], c['quality_cutoff']): c for c in json.load(f)['cases']}


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted((c.name, q) for c in ppc.cases() for q in ppc.Q_CUTOFFS)
    for c in ppc.cases():
        for q in ppc.Q_CUTOFFS:
            assert golden[(c.name, q)]['sam'] == c.sha(), c.name   # the generator has not drifted


@pytest.mark.parametrize('q', ppc.Q_CUTOFFS)
def test_oracle_equals_reference_counters(golden, q):
    for c in ppc.cases():
        want = golden[(c.name, q)]
        refmap, _ = oracle.pileup(c.ref_names, c.pairs, q)
        assert list(refmap) == want['order'], c.name
        ppc.assert_equals_stored(ppc.canonical_counters(refmap), want['counters'], c.name)
        conseqs = oracle.sam_to_conseqs(c.sam.splitlines(True), q)
        assert list(conseqs) == list(want['conseqs']), c.name
        for name, text in conseqs.items():
            ppc.assert_equals_stored(text, want['conseqs'][name], (c.name, name))


def test_tokens_big_construction_matches_oracle():
    """tokens_big's arrays, at 2 000 pairs, leave exactly the tokens the
    oracle counts: the expected keys of the full-size case are sound."""
    args, ref_lens, (uniq, count) = ppc.tokens_big(2000)
    ref_names, pairs = ppc.tokens_big_pairs(args)
    refmap, counts = oracle.pileup(ref_names, pairs, 20)
    assert counts['r1'] == 2000
    got = {}
    for pos, c in refmap['r1'][0].items():
        for tok, n in c.items():
            if len(tok) > 1:
                assert len(tok) == 7
                key = pos
                for ch in tok:
                    key = key * 4 + 'ACGT'.index(ch)
                got[key] = n
    assert got == dict(zip(uniq.tolist(), count.tolist()))
    assert sum(got.values()) == 2000 and max(got.values()) == 2

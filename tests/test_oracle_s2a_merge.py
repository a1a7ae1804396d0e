"""The oracle restatement of sam2aln (oracle/og_sam2aln.py) on the directed
texts of tests/s2a_merge_cases.py, pinned to the reference's own outputs
(tests/golden/s2a_merge_paths.json, written by tests/golden/gen_s2a_merge.py).
No GPU: this is where the cases' preconditions are checked -- the generators
assert their own when they build the texts, and here every targeted unit is
shown to reach aligned.csv in the reference."""
import pytest

import og_sam2aln
import s2a_merge_cases as mc


def _oracle(text, cuts):
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = list(cuts)
    try:
        return og_sam2aln.sam2aln(text)
    finally:
        og_sam2aln.Q_CUTOFFS = saved


def test_fixture_holds_every_case_and_nothing_else():
    fx = mc.fixture()
    assert sorted(fx) == sorted(c.name for c in mc.cases())
    for c in mc.cases():
        lists = [] if c.refused else c.lists
        assert [r['q_cutoffs'] for r in fx[c.name]['runs']] == lists, c.name


@pytest.mark.parametrize('c', mc.cases(), ids=lambda c: c.name)
def test_generated_input_is_the_fixtures(c):
    """A generator that drifted asks for a regenerated fixture."""
    assert c.sha() == mc.fixture()[c.name]['input'], \
        '{}: run tests/golden/gen_s2a_merge.py'.format(c.name)


@pytest.mark.parametrize('run', mc.runs(), ids=mc.run_id)
def test_oracle_equals_reference(run):
    c, cuts = run
    want = mc.want_of(run)
    if c.raises:
        with pytest.raises(Exception) as err:
            _oracle(c.text, cuts)
        assert type(err.value).__name__ == want['raises']['class']
        assert str(err.value) == want['raises']['message']
        return
    assert 'raises' not in want
    got = _oracle(c.text, cuts)
    for name, text in zip(('aligned', 'insert', 'failed'), got):
        mc.assert_equals_stored(text, want[name], (c.name, cuts, name))
    assert [t.count('\n') - 1 for t in got] == want['rows']


@pytest.mark.parametrize('run', [r for r in mc.runs() if not r[0].raises], ids=mc.run_id)
def test_targeted_units_reach_aligned_csv(run):
    """A condition on the inputs: failed.csv of the reference holds exactly
    the units the generator names (none but in `status` and `unpaired`), and
    aligned.csv counts every other unit once per cutoff."""
    c, cuts = run
    want = mc.want_of(run)
    assert isinstance(want['failed'], str), 'failed.csv too long to store'
    failed = [line.split(',')[0] for line in want['failed'].splitlines()[1:]]
    assert len(failed) == len(set(failed)) and set(failed) == set(c.failing), (c.name, cuts)
    if c.name not in ('status', 'unpaired'):
        assert not failed
    # counts of aligned.csv (from the oracle's text, equal to the reference's by the test above)
    al = _oracle(c.text, cuts)[0]
    total = sum(int(line.split(',')[3]) for line in al.splitlines()[1:])
    host_failed = len(mc.units_of(c.text)) - len(c.units)
    many_ns = len(failed) - host_failed
    assert total >= (len(c.units) - many_ns) * len(set(cuts))
    if not many_ns:
        assert total == len(c.units) * len(set(cuts))

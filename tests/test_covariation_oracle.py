"""tests/covariation_oracle.py, the plain-Python statement of covariation.csv,
without a device: the hand-worked cases, its one-variant columns against
tests/linkage_oracle.py on one-position sets, and a golden case through the
oracle Report's coordinate map."""
import gzip
import os
import random

import pytest

import covariation_cases as cases
import covariation_oracle as co
import linkage_oracle as lo

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')


def test_the_masks_of_the_cases_are_the_oracles():
    assert cases.CALLED == co.CALLED_MASK
    assert all(cases.bit(ch) == 1 << co.CODES.index(ch) for ch in co.CODES[1:])
    assert len(co.CALLED) == 22 and set(co.CALLED) < set(co.CODES) and 'X' not in co.CALLED and '?' not in co.CALLED


@pytest.mark.parametrize('name', sorted(cases.GRAM))
def test_hand_worked_gram(name):
    rows, cols, gram = cases.GRAM[name]
    assert co.gram(rows, cols) == gram
    assert all(gram[i][j] == gram[j][i] for i in range(len(cols)) for j in range(len(cols)))


@pytest.mark.parametrize('name', sorted(cases.SELECT))
def test_hand_worked_selection(name):
    tallies, min_fraction, min_count, max_variants, kept, dropped = cases.SELECT[name]
    assert co.select(tallies, min_fraction, min_count, max_variants) == (kept, dropped)


def test_hand_worked_pairs():
    records = co.pairs(cases.PAIR_ROWS, cases.PAIR_VARIANTS, cases.PAIR_PLACE, 1)
    assert records == cases.PAIR_RECORDS
    assert [co.line('s', '15', r) for r in records] == cases.PAIR_LINES
    # n >= min_count: both pairs have n = 10
    assert co.pairs(cases.PAIR_ROWS, cases.PAIR_VARIANTS, cases.PAIR_PLACE, 10) == cases.PAIR_RECORDS
    assert co.pairs(cases.PAIR_ROWS, cases.PAIR_VARIANTS, cases.PAIR_PLACE, 11) == []


@pytest.mark.parametrize('counts', sorted(cases.MEASURES))
def test_direction_and_r2(counts):
    assert (co.direction(*counts), co.r2(*counts)) == cases.MEASURES[counts]


def test_one_variant_columns_are_one_position_linkage_sets():
    """The diagonal of a one-character column is what linkage counts for that
    character at a one-position set, the called column's is the called
    characters' sum, and a pair of one-character columns is the two-position
    haplotype's count."""
    rng = random.Random(11)
    rows = [(rng.randint(0, 12), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(1, 40))),
             rng.randint(1, 30)) for _ in range(150)]
    seen = set()
    for frame in range(3):
        for codon in (1, 4, 9, 30):
            found, coverage = lo.count(rows, frame, [codon])
            cols = [(frame, codon, 1 << k) for k in range(1, 25)] + [(frame, codon, co.CALLED_MASK)]
            gram = co.gram(rows, cols)
            assert [gram[k][k] for k in range(24)] == [found.get(ch, 0) for ch in co.CODES[1:]]
            assert gram[24][24] == sum(n for ch, n in found.items() if ch in co.CALLED)
            assert sum(gram[k][k] for k in range(24)) == coverage
            # two characters of one codon never share a row
            assert all(gram[i][j] == 0 for i in range(24) for j in range(24) if i != j)
            seen.update(found)
    assert {'X', '?', '-'} <= seen
    two, _ = lo.count(rows, 1, [2, 5])
    assert len(two) > 5
    for hap, n in two.items():
        a, b = (1 << co.CODES.index(ch) for ch in hap)
        assert co.gram(rows, [(1, 2, a), (1, 5, b)])[0][1] == n


def test_a_golden_case_selects_nothing_at_the_defaults():
    """The committed goldens carry no real minority variants."""
    with gzip.open(os.path.join(E2E_DIR, 'c1_example', 'aligned.csv.gz'), 'rt') as f:
        lines, runs = co.expected(f.read())
    assert lines == [] and runs and all(kept == [] and dropped == 0 for _s, _q, kept, dropped, _r in runs)

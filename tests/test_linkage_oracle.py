"""tests/linkage_oracle.py, the plain-Python statement of linkage.csv, without
a device: the hand-worked cases, one-position sets against the codon classes
of tests/amino_detail_oracle.py, and RT 103 of a golden case against the
golden amino.csv through the oracle Report's coordinate map."""
import csv
import gzip
import io
import os
import random

import pytest

import amino_detail_oracle as ado
import linkage_cases
import linkage_oracle as lo
import og_aln2counts as og

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')


@pytest.mark.parametrize('name', sorted(linkage_cases.CASES))
def test_hand_worked_cases(name):
    rows, sets, min_count, entries, coverage = linkage_cases.CASES[name]
    assert lo.entries(rows, sets, min_count) == (entries, coverage)


def test_cases_cover_every_character_kind():
    seen = set(b''.join(e[2] for case in linkage_cases.CASES.values() for e in case[3]).decode())
    assert {'*', '-', '?', 'X', 'K'} <= seen


@pytest.mark.parametrize('seed', [1, 2])
def test_one_position_sets_are_the_codon_classes(seed):
    """For a set of one codon the counts per character are the classes
    amino_detail.csv counts there, and coverage is their sum."""
    rng = random.Random(seed)
    rows = [(rng.randint(0, 40), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(1, 60))),
             rng.randint(1, 50)) for _ in range(120)]
    cells = ado.tally(rows)
    kinds = set()
    for frame in range(3):
        top = max(j for f, j in cells if f == frame)
        for j in range(top + 3):             # two codons past every row as well
            found, coverage = lo.count(rows, frame, [j])
            cell = cells.get((frame, j), {})
            want = {k: cell.get(k, 0) for k in ('letter', 'X', 'partial', 'del')}
            got = {'letter': sum(n for h, n in found.items() if h in og.AMINOS), 'X': found.get('X', 0),
                   'partial': found.get('?', 0), 'del': found.get('-', 0)}
            assert got == want, (frame, j)
            assert coverage == sum(want.values()) == sum(found.values())
            assert all(len(h) == 1 for h in found)
            kinds.update(found)
    assert {'X', '?', '-', '*'} <= kinds and len(kinds) > 20


def test_letters_are_the_translations():
    """The letters of a one-codon set are what AminoTally.count_aminos counts."""
    rng = random.Random(7)
    rows = [(0, ''.join(rng.choice('ACGT') for _ in range(9)), rng.randint(1, 9)) for _ in range(200)]
    for j in range(3):
        tally = og.AminoTally(j)
        for _off, seq, n in rows:
            tally.count_aminos(seq[3 * j:3 * j + 3], n)
        assert lo.count(rows, 0, [j])[0] == dict(tally.counts)


def _gz(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.csv.gz'), 'rt') as f:
        return f.read()


def test_rt_103_of_a_golden_case_is_its_amino_csv_row():
    aligned = _gz('syn_pol_indel', 'aligned')
    lines, unplaced, tallies = lo.expected(aligned, {'RT': [[103]], 'no such region': [[1]]})
    assert not unplaced
    golden = [r for r in csv.reader(io.StringIO(_gz('syn_pol_indel', 'a2c_amino')))
              if r[1] == 'RT' and r[4] == '103']
    assert len(golden) == len(tallies) >= 1
    for row in golden:
        found, coverage = tallies[row[0], row[2], 'RT', 0]
        assert [found.get(a, 0) for a in og.AMINOS] == [int(x) for x in row[5:26]]
        assert sum(int(x) for x in row[5:26]) > 0
        assert coverage >= sum(int(x) for x in row[5:26])
    assert all(line[1] == 'RT' and line[3] == '103' for line in lines)
    assert [line[:3] + line[4:] for line in lines] == [
        [seed, 'RT', qcut, h, str(n), str(tallies[seed, qcut, 'RT', 0][1])]
        for (seed, qcut, _r, _s), (found, _c) in tallies.items() for h, n in lo.ordered(found)]


def test_min_count_cuts_rows_not_coverage():
    rows = [(0, 'AAA', 5), (0, 'AGA', 1), (0, 'ANA', 1)]
    assert lo.entries(rows, [(0, [0])], 2) == ([(0, 5, b'K')], [7])
    assert lo.entries(rows, [(0, [0])], 1) == ([(0, 5, b'K'), (0, 1, b'R'), (0, 1, b'X')], [7])

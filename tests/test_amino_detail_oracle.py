"""tests/amino_detail_oracle.py, the specification of amino_detail.csv's codon
classes, pinned without a GPU: on the goldens every codon a row visits lands
in exactly one of letter / X / partial / del / blank, the letters being the
ones the oracle's Report counts; and the hand-worked cases of
tests/amino_detail_cases.py give their literal numbers."""
import gzip
import io
import os

import pytest

import amino_detail_cases
import amino_detail_oracle as ado
import og_aln2counts as og

E2E_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'e2e')


def _aligned(case):
    with gzip.open(os.path.join(E2E_DIR, case, 'aligned.csv.gz'), 'rt') as f:
        return f.read()


@pytest.mark.parametrize('case', ['c1_example', 'syn_pol_indel', 'syn_hiv3', 'syn_unpaired300'])
def test_the_classes_partition_every_codon_read(case):
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    rep._map = lambda name, ref: None         # only read()'s seed_aminos are looked at
    translate, seen = og.translate, {}

    def memo(*args):
        if args not in seen:
            seen[args] = translate(*args)
        return seen[args]
    og.translate = memo
    cells_seen = classes_seen = 0
    try:
        for group in ado.groups(_aligned(case)):
            rep.read(group)
            cells = ado.tally(group)
            visits = {}
            for row in group:
                off, n, count = int(row['offset']), len(row['seq']), int(row['count'])
                for f in range(3):
                    for j in range(off // 3, -(-(f + off + n) // 3)):
                        visits[f, j] = visits.get((f, j), 0) + count
            assert set(cells) == set(visits)
            for (f, j), total in visits.items():
                cell = cells[f, j]
                letters = sum(rep.seed_aminos[f][j].counts.values())
                assert cell.get('letter', 0) == letters
                assert letters + sum(cell.get(k, 0) for k in ado.CLASSES + ('blank',)) == total
                classes_seen += sum(1 for k in ado.CLASSES if cell.get(k, 0))
            cells_seen += len(visits)
    finally:
        og.translate = translate
    assert cells_seen > 500 and classes_seen > 500


@pytest.mark.parametrize('name', sorted(amino_detail_cases.CASES))
def test_hand_worked_cases(name):
    rows, want = amino_detail_cases.CASES[name]
    assert sorted(want) == [0, 1, 2]
    for frame, table in want.items():
        ncod = max(-(-(frame + off + len(seq)) // 3) for off, seq, _ in rows)
        assert len(table) == ncod
        assert ado.table(rows, frame, ncod) == table, (name, frame)


def test_header_is_amino_csvs_then_the_six_columns():
    assert ado.HEADER[:26] == ['seed', 'region', 'q-cutoff', 'query.aa.pos', 'refseq.aa.pos'] + list(og.AMINOS)
    assert ado.HEADER[26:] == ['X', 'partial', 'del', 'ins', 'clip', 'coverage']

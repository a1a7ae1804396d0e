"""aln2counts' covariation.csv: which minority variants single reads carry
together, every pair at once, counted on the device (k_a2c_gram_bits /
k_a2c_gram_pairs through mh_a2c_gram; SequenceReport.count_covariation,
aln2counts(covariation_csv=)).

1. The device call against tests/covariation_oracle.py on rows loaded with
   a2c_load_rows, compared exactly: the hand-worked cases, rows per group
   around the 64-row word and the pair kernel's row slice, columns around the
   64-column tile up to the 512 of a call, frames, masks, row edges, count
   planes, random rows, bad requests.
2. The same call against the existing kernels: amino_detail.csv's counts and
   linkage.csv's two-position haplotypes.
3. The file against the oracle's on an input with planted variants; the
   resident chain; two ranks."""
import csv
import gzip
import io
import json
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest

import amino_detail_oracle as ado
import covariation_cases as cases
import covariation_oracle as co
import linkage_oracle as lo
import og_aln2counts as og
from micall_amd import _native, session
from micall_amd import aln2counts as a2c
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
WORKER = os.path.join(HERE, 'gpu_covariation_worker.py')
SLOT = 2
SLICE_ROWS = 64 * 32          # A2C_GRAM_SLICE row words of 64 rows: what a block of k_a2c_gram_pairs stages at once
MAX_COLUMNS = 512             # A2C_GRAM_MAX
PLAIN = ('nuc', 'amino', 'coord_ins', 'conseq')
SHIFTED = 'syn_pol_indel+1'
# (region, position) -> which rows (by index in the file) get TGG written over the codon
PLANTED = {('RT', 100): lambda i: i % 3 == 0, ('RT', 151): lambda i: i % 3 == 0 or i % 5 == 0,
           ('RT', 184): lambda i: i % 3 == 1, ('PR', 90): lambda i: i % 2 == 0}
_CACHE = {}


# ---------------------------------------------------------------------------
# 1. the device call against the oracle
# ---------------------------------------------------------------------------
def _load(groups, slot=SLOT):
    ctx = session.context()
    rows = [r for grp in groups for r in grp]
    first = [0]
    for grp in groups:
        first.append(first[-1] + len(grp))
    ctx.a2c_load_rows(slot, [r[1] for r in rows], [r[0] for r in rows], [r[2] for r in rows], first,
                      a2c._CODON_CHARS)
    return ctx


def _check(rows, cols, groups=None, g=0):
    """mh_a2c_gram over group g (rows) against the oracle; returns (gram as
    lists, stats)."""
    ctx = _load(groups or [rows])
    got, stats = ctx.a2c_gram(SLOT, g, cols)
    assert got.shape == (len(cols), len(cols)) and got.dtype == np.int64
    assert got.tolist() == co.gram(rows, cols)
    assert stats['rows'] == len(rows) and stats['words'] == -(-len(rows) // 64)
    assert stats['sites'] == len({c[:2] for c in cols})
    tiles = -(-len(cols) // 64)
    assert stats['tiles'] == tiles * (tiles + 1) // 2
    planes = 0
    for r in rows:
        planes |= r[2]
    assert stats['planes'] == bin(planes).count('1')
    return got.tolist(), stats


def _codon_of_each_character():
    """A codon text for each of the 24 characters (tests/test_gpu_linkage.py's)."""
    found = {}
    for a in 'ACGT':
        for b in 'ACGT':
            for c in 'ACGT':
                found.setdefault(og.translate(a + b + c), a + b + c)
    assert sorted(found) == sorted(og.AMINOS)
    found.update({'X': 'ANA', '?': 'A-A', '-': '---'})
    return found


def _random_rows(rng, n, alphabet='ACGTN-n', lengths=(5, 40, 90, 151), counts=(1, 4)):
    return [(rng.choice((0, 1, 2, 7, 30, 31)) + rng.randrange(0, 3) * 3,
             ''.join(rng.choice(alphabet) for _ in range(rng.choice(lengths))), rng.randint(*counts))
            for _ in range(n)]


def _random_mask(rng):
    return sum(1 << k for k in rng.sample(range(1, 25), rng.choice((1, 1, 2, 5, 22))))


@pytest.mark.parametrize('name', sorted(cases.GRAM))
def test_hand_worked_cases(name):
    rows, cols, gram = cases.GRAM[name]
    got, _ = _check(rows, cols)
    assert got == gram


def test_hand_worked_pairs_from_the_columns_a_report_passes():
    """One called column per codon, one column per variant: the four counts of
    the hand-worked pairs are cells of the matrix."""
    sites = [(0, 0), (0, 1)]
    variants = [(0, 0, 'R'), (0, 1, 'W'), (0, 1, '-')]
    cols = [(f, k, co.CALLED_MASK) for f, k in sites] + [(f, k, cases.bit(ch)) for f, k, ch in variants]
    got, _ = _check(cases.PAIR_ROWS, cols)
    assert [(got[0][1], got[2][1], got[0][b], got[2][b]) for b in (3, 4)] == [r[6:] for r in cases.PAIR_RECORDS]


@pytest.mark.parametrize('n', [1, 63, 64, 65, SLICE_ROWS - 1, SLICE_ROWS, SLICE_ROWS + 1])
def test_rows_per_group(n):
    """One row below, at and above the 64-row word and the pair kernel's row
    slice; the last row differs from the others, so a lost last row shows."""
    rng = random.Random(n)
    rows = [(rng.randrange(0, 7), ''.join(rng.choice('ACGT-') for _ in range(rng.randint(6, 14))), rng.randint(1, 9))
            for _ in range(n - 1)] + [(0, 'TGGTGGTGGTGG', 11)]
    cols = [(0, 1, co.CALLED_MASK), (0, 1, cases.bit('W')), (0, 2, cases.bit('W')), (1, 2, co.CALLED_MASK),
            (2, 3, _random_mask(rng)), (0, 3, co.CALLED_MASK)]
    got, stats = _check(rows, cols)
    assert got[1][2] >= 11 and stats['words'] == -(-n // 64)


@pytest.mark.parametrize('n_cols', [1, 2, 63, 64, 65, MAX_COLUMNS - 1, MAX_COLUMNS])
def test_columns_per_call(n_cols):
    """One below, at and above the 64-column tile, and up to the most a call
    takes: three frames, codons with one and with several columns."""
    rng = random.Random(n_cols)
    rows = _random_rows(rng, 140, alphabet='ACGTACGTACGTN-', lengths=(60, 151), counts=(1, 3))
    cols = [(rng.randrange(3), rng.randrange(0, 55), _random_mask(rng)) for _ in range(n_cols)]
    got, stats = _check(rows, cols)
    assert any(got[k][k] for k in range(n_cols))
    if n_cols > 2:
        assert stats['sites'] < n_cols or n_cols < 64
        assert any(got[i][j] for i in range(n_cols) for j in range(i)), 'no pair shares a row'


def test_one_column_more_than_a_call_takes_is_refused():
    ctx = _load([[(0, 'AAATTT', 1)]])
    with pytest.raises(_native.NativeError, match='513 columns'):
        ctx.a2c_gram(SLOT, 0, [(0, 0, 2)] * (MAX_COLUMNS + 1))
    assert ctx.a2c_gram(SLOT, 0, [(0, 0, cases.bit('K'))] * MAX_COLUMNS)[0].tolist() == [[1] * MAX_COLUMNS] * MAX_COLUMNS


def test_second_group_of_a_slot():
    """The second group's first row is row 3 of the slot: not word-aligned."""
    first = [(0, 'GGGGGGGGG', 9)] * 3
    rng = random.Random(5)
    second = [(3, 'AAATTT', 2), (0, 'CCCAAATTT', 1), (3, 'AGA', 4)] + _random_rows(rng, 130, lengths=(5, 40))
    cols = [(0, 1, cases.bit('K')), (0, 2, cases.bit('F')), (0, 0, cases.bit('P')), (0, 1, co.CALLED_MASK)]
    got, _ = _check(second, cols, groups=[first, second], g=1)
    assert got[0][1] >= 3 and got[2][0] >= 1
    got, _ = _check(first, [(0, 1, cases.bit('G')), (0, 2, co.CALLED_MASK)], groups=[first, second], g=0)
    assert got == [[27, 27], [27, 27]]


def test_frames_in_one_call_and_equal_columns():
    rng = random.Random(3)
    rows = _random_rows(rng, 300, lengths=(3, 30, 160), counts=(1, 9))
    rows += [(0, ''.join(rng.choice('ACGT') for _ in range(150)), 7), (1, 'ACGTTGCA' * 19, 5), (2, 'CCGATA' * 25, 3)]
    cols = [(f, k, m) for f in range(3) for k in (0, 20, 21, 41) for m in (co.CALLED_MASK, _random_mask(rng))]
    cols += [cols[1], cols[1], cols[-1]]
    got, _ = _check(rows, cols)
    n = len(cols)
    assert got[1] == got[n - 3] == got[n - 2] and got[1][n - 3] == got[1][1] > 0
    assert all(any(got[k][k] > 0 for k in range(8 * f, 8 * f + 8, 2)) for f in range(3))


def test_each_of_the_24_one_bit_masks():
    codon = _codon_of_each_character()
    chars = co.CODES[1:]
    rows = [(0, 'AAA' + codon[ch] + 'CCC', 3 + k) for k, ch in enumerate(chars)]
    cols = [(0, 1, 1 << (k + 1)) for k in range(24)] + [(0, 1, co.CALLED_MASK), (0, 0, cases.bit('K'))]
    got, _ = _check(rows, cols)
    assert [got[k][k] for k in range(24)] == [3 + k for k in range(24)]
    assert all(got[i][j] == 0 for i in range(24) for j in range(24) if i != j)
    assert got[24][24] == sum(3 + k for k, ch in enumerate(chars) if ch in co.CALLED)
    assert got[25][:24] == [3 + k for k in range(24)]


def test_row_edges():
    # a row ending inside a codon, a row starting inside one: partial, not called
    got, _ = _check([(0, 'AAAGGGT', 2), (1, 'AAGGGTTT', 3)],
                    [(0, 0, cases.bit('K')), (0, 0, cases.bit('?')), (0, 1, cases.bit('G')), (0, 2, cases.bit('?')),
                     (0, 2, cases.bit('F')), (0, 2, co.CALLED_MASK)])
    assert [got[k][k] for k in range(6)] == [2, 3, 5, 2, 3, 3]
    # offset % 3 + frame >= 3: the first codon the row reaches is padding only
    got, _ = _check([(2, 'GAAATTT', 1), (5, 'AAATTT', 2)],
                    [(1, 0, 0x1fffffe), (1, 1, 0x1fffffe), (2, 1, 0x1fffffe), (2, 2, 0x1fffffe), (2, 3, 0x1fffffe)])
    assert [got[k][k] for k in range(5)] == [0, 1, 1, 3, 3]
    # three '-' of the row are a deletion, the padding's are blank
    got, _ = _check([(0, 'AAA---TTT', 4), (6, 'TTT', 1), (0, 'AAA', 2)],
                    [(0, 1, cases.bit('-')), (0, 1, 0x1fffffe), (0, 2, cases.bit('F')), (0, 0, cases.bit('K'))])
    assert got == [[4, 4, 4, 4], [4, 4, 4, 4], [4, 4, 5, 4], [4, 4, 4, 6]]
    # 'nnn' is blank, 'nAn' is partial; TAA is '*', ANA is X
    got, _ = _check([(0, 'TAAnnnANA', 1), (0, 'TAAnAnANA', 2)],
                    [(0, 1, 0x1fffffe), (0, 1, cases.bit('?')), (0, 0, cases.bit('*')), (0, 2, cases.bit('X')),
                     (0, 2, co.CALLED_MASK)])
    assert [got[k][k] for k in range(5)] == [2, 2, 3, 3, 0] and got[0][2] == 2
    # a codon beyond every row, alone and beside one that is read
    got, stats = _check([(0, 'AAATTT', 5), (30, 'ACGT', 1)],
                        [(0, 400, 0x1fffffe), (0, 0, cases.bit('K')), (2, 2 ** 31 - 1, co.CALLED_MASK)])
    assert got == [[0, 0, 0], [0, 5, 0], [0, 0, 0]] and stats['sites'] == 3


def test_count_planes():
    """Counts 1 .. 9 set four planes, bit 30 a fifth; cells are exact sums."""
    rng = random.Random(9)
    rows = [(0, rng.choice(('AAATTT', 'AGATTT', 'AAATTC', 'AGA')), 1 + k % 9) for k in range(200)]
    cols = [(0, 0, cases.bit('K')), (0, 0, cases.bit('R')), (0, 1, cases.bit('F')), (0, 1, co.CALLED_MASK)]
    _, stats = _check(rows, cols)
    assert stats['planes'] == 4
    rows.append((0, 'AAATTT', (1 << 30) + 5))
    got, stats = _check(rows, cols)
    assert stats['planes'] == 5 and got[0][2] > 1 << 30
    _, stats = _check([(0, 'AAATTT', 2 ** 32 - 1)], cols)
    assert stats['planes'] == 32


def test_a_cell_close_to_two_to_the_32():
    """5 000 rows x 850 000 = 4.25e9 in one cell, above 2**31 and just below
    the 2**32 - 1 that a group's counts may add up to; 5 000 x 1 000 000 is
    refused by the load (as every load refuses it), so no cell of a loaded
    group can exceed 2**32."""
    rows = [(0, 'AAATTT', 850000)] * 5000
    ctx = _load([rows])
    got, stats = ctx.a2c_gram(SLOT, 0, [(0, 0, cases.bit('K')), (0, 1, cases.bit('F')), (0, 1, cases.bit('L'))])
    assert got.tolist() == [[4250000000, 4250000000, 0], [4250000000, 4250000000, 0], [0, 0, 0]]
    assert 2 ** 31 < got[0][1] < 2 ** 32 and stats['rows'] == 5000
    with pytest.raises(_native.NativeError, match='add up to more than'):
        _load([[(0, 'AAATTT', 1000000)] * 5000])


def test_random_rows():
    rng = random.Random(20)
    rows = _random_rows(rng, 4000)
    cols = [(rng.randrange(3), rng.randrange(0, 45), _random_mask(rng)) for _ in range(40)]
    got, stats = _check(rows, cols)
    assert sum(got[i][j] > 0 for i in range(40) for j in range(i)) > 300
    assert stats['planes'] == 3 and stats['words'] == 63


def test_bad_requests_are_refused_and_leave_nothing_behind():
    ctx = _load([[(0, 'AAATTT', 1)]])
    ok = [(0, 0, cases.bit('K')), (0, 1, cases.bit('F'))]
    zeros = dict.fromkeys(_native.Context.GRAM_STATS, 0)
    assert ctx.a2c_gram_stats(SLOT) == dict(zeros, ms=0.0)       # a load clears them
    for cols in ([], [(3, 0, 2)], [(-1, 0, 2)], [(0, -1, 2)], [(0, 0, 0)], [(0, 0, 1)], [(0, 0, 3)],
                 [(0, 0, 1 << 25)], [(0, 0, 1 << 31)], ok + [(0, 0, (1 << 25) | 2)]):
        got, stats = ctx.a2c_gram(SLOT, 0, ok)
        assert got.tolist() == [[1, 1], [1, 1]] and stats['rows'] == 1
        with pytest.raises(_native.NativeError):
            ctx.a2c_gram(SLOT, 0, cols)
        stale = ctx.a2c_gram_stats(SLOT)
        assert {k: stale[k] for k in zeros} == zeros, cols
    for g in (1, -1):
        with pytest.raises(_native.NativeError, match='no group'):
            ctx.a2c_gram(SLOT, g, ok)
    assert ctx.a2c_gram(SLOT, 0, ok)[0].tolist() == [[1, 1], [1, 1]]
    # a load that failed leaves the slot without one
    with pytest.raises(_native.NativeError):
        ctx.a2c_load_rows(SLOT, ['AXA'], [0], [1], [0, 1], a2c._CODON_CHARS)
    with pytest.raises(_native.NativeError, match='nothing is loaded'):
        ctx.a2c_gram(SLOT, 0, ok)


# ---------------------------------------------------------------------------
# 2. against the existing kernels
# ---------------------------------------------------------------------------
def _gz(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.csv.gz'), 'rt') as f:
        return f.read()


def _rows(text):
    return list(csv.reader(io.StringIO(text)))


def _oracle_report(text):
    group = ado.groups(text)[0]
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    rep.read(group)
    return rep, group


def _run(aligned_handle, covariation=True, **kw):
    outs = {k: io.StringIO() for k in PLAIN + ('covariation', 'amino_detail', 'linkage')}
    if covariation:
        kw['covariation_csv'] = outs['covariation']
    if kw.pop('detail', False):
        kw['amino_detail_csv'] = outs['amino_detail']
    if 'linkage_positions' in kw:
        kw['linkage_csv'] = outs['linkage']
    a2c.aln2counts(aligned_handle, outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'], **kw)
    return {k: v.getvalue() for k, v in outs.items()}


def test_the_matrix_against_amino_detail_and_linkage():
    """After one aln2counts call on syn_pol_indel, with its rows still in the
    report's slot: the 22 one-character columns of every PR position have
    amino_detail.csv's counts on the diagonal (k_a2c_gram_* against k_a2c_count
    and k_a2c_detail), and two one-bit columns share what linkage.csv counts
    for that two-position haplotype (against k_a2c_link)."""
    text = _gz('syn_pol_indel', 'aligned')
    linked_sets = {'PR': [[30, 46], [82, 90]], 'RT': [[41, 67], [103, 184]]}
    got = _run(io.StringIO(text), covariation=False, detail=True, linkage_positions=linked_sets)
    rep, _group = _oracle_report(text)
    ctx = session.context()
    detail = [r for r in _rows(got['amino_detail'])[1:] if r[1] == 'PR' and r[3] != '']
    assert len(detail) > 90
    frame = rep.reading_frames['PR']
    checked = 0
    for at in range(0, len(detail), 23):                    # 23 positions x 22 characters = 506 columns
        part = detail[at:at + 23]
        cols = [(frame, int(r[3]) - 1, bit) for r in part for bit in a2c._COVAR_BIT]
        gram = ctx.a2c_gram(a2c.SLOT_REPORT, 0, cols)[0]
        for k, r in enumerate(part):
            want = [int(x) for x in r[5:26]] + [int(r[28])]        # the 21 letters, del
            assert gram.diagonal()[22 * k:22 * k + 22].tolist() == want, r[4]
            checked += sum(want) > 0
    assert checked > 90
    pairs = 0
    for seed, region, qcut, where, hap, count, _coverage in _rows(got['linkage'])[1:]:
        f, codons = lo.place(rep, region, [int(p) for p in where.split(';')])
        cols = [(f, k, cases.bit(ch)) for k, ch in zip(codons, hap)]
        assert ctx.a2c_gram(a2c.SLOT_REPORT, 0, cols)[0][0][1] == int(count), (region, where, hap)
        pairs += 1
    assert pairs > 8


# ---------------------------------------------------------------------------
# 3. the file
# ---------------------------------------------------------------------------
def _planted(shift=0):
    """(text, indices of the rows changed): syn_pol_indel's aligned.csv with
    every count 1 and TGG written over the codons of PLANTED wherever the
    codon lies whole inside the row and reads as a letter; shift moves every
    offset right (SHIFTED: the regions read in frame 2)."""
    if shift in _CACHE:
        return _CACHE[shift]
    text = _gz('syn_pol_indel', 'aligned')
    rep, group = _oracle_report(text)
    assert len(ado.groups(text)) == 1
    head = text.split('\n', 1)[0].split(',')
    assert head == ['refname', 'qcut', 'rank', 'count', 'offset', 'seq']
    lines, changed = [head], set()
    for i, row in enumerate(group):
        offset, seq = int(row['offset']), row['seq']
        for (region, pos), chosen in PLANTED.items():
            frame, (codon,) = lo.place(rep, region, [pos])
            at = 3 * codon - frame - offset
            if chosen(i) and at >= 0 and at + 3 <= len(seq) and \
                    lo.haplotype(offset, seq, frame, [codon]) in tuple(og.AMINOS):
                seq = seq[:at] + 'TGG' + seq[at + 3:]
                changed.add(i)
        lines.append([row['refname'], row['qcut'], row['rank'], '1', str(offset + shift), seq])
    out = io.StringIO()
    csv.writer(out, lineterminator='\n').writerows(lines)
    _CACHE[shift] = out.getvalue(), sorted(changed)
    return _CACHE[shift]


def _expected(shift=0, **kw):
    key = (shift, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = co.expected(_planted(shift)[0], **kw)
    return _CACHE[key]


def _file(lines):
    out = io.StringIO()
    csv.writer(out, lineterminator=os.linesep).writerows([co.HEADER] + lines)
    return out.getvalue()


def test_the_planted_input_holds_what_the_comparison_needs():
    """By the oracle alone: the frames and the map are syn_pol_indel's, the
    four planted variants are the ones selected, and the pairs cover n.ab =
    n.a, n.ab = 0, a pair across regions and one below min_count."""
    text, changed = _planted()
    rep0, _ = _oracle_report(_gz('syn_pol_indel', 'aligned'))
    rep1, _ = _oracle_report(text)
    assert rep0.reading_frames == rep1.reading_frames
    for region in rep0.reports:
        assert [(t.consensus_index, p) for t, p in rep0.reports[region]] == \
               [(t.consensus_index, p) for t, p in rep1.reports[region]]
    lines, runs = _expected()
    assert len(runs) == 1 and len(changed) > 40
    _seed, _qcut, kept, dropped, records = runs[0]
    assert kept == [('PR', 90, 'W'), ('RT', 100, 'W'), ('RT', 151, 'W'), ('RT', 184, 'W')] and dropped == 0
    tallies, _place = co.run_tallies(rep1, ado.groups(text)[0])
    assert [tallies[v[:2]]['W'] for v in kept] == [40, 24, 39, 29]
    by_pair = {(r[0], r[1], r[3], r[4]): r[6:] for r in records}
    assert by_pair['RT', 100, 'RT', 151] == (46, 13, 19, 13)          # n.ab == n.a > 0
    n, _na, _nb, nab = by_pair['RT', 100, 'RT', 184]
    assert nab == 0 and n >= 10
    assert by_pair['PR', 90, 'RT', 100][0] == 14                      # across regions, written
    assert ('PR', 90, 'RT', 184) not in by_pair                       # n = 1 < min_count
    assert co.pairs(ado.groups(text)[0], kept, _place, 1)[2][6] == 1
    assert len(lines) == len(records) == 4                            # PR 90 / RT 151 has n = 5


@pytest.mark.parametrize('shift', [0, 1])
def test_covariation_file_matches_the_oracle(shift):
    text = _planted(shift)[0]
    if shift:
        assert set(_oracle_report(text)[0].reading_frames.values()) == {2}
    lines, runs = _expected(shift)
    assert len(lines) >= 4 and [r[2] for r in runs] == [_expected()[1][0][2]]
    got = _run(io.StringIO(text))
    assert got['covariation'] == _file(lines)
    plain = _run(io.StringIO(text), covariation=False)
    assert all(got[k] == plain[k] for k in PLAIN) and plain['covariation'] == ''


def test_more_variants_than_the_cap_keeps_the_most_counted():
    text, _ = _planted()
    kw = dict(min_fraction=0.001, min_count=1, max_variants=8)
    lines, runs = _expected(**kw)
    _seed, _qcut, kept, dropped, records = runs[0]
    assert len(kept) == 8 and dropped > 0 and len(lines) > 4
    got = _run(io.StringIO(text), **{'covariation_' + k: v for k, v in kw.items()})
    assert got['covariation'] == _file(lines)
    report = a2c.SequenceReport(a2c.InsertionWriter(io.StringIO()), a2c.project_config.ProjectConfig.loadDefault(),
                                a2c.CONSEQ_MIXTURE_CUTOFFS)
    report.read(ado.groups(text)[0])
    assert report.count_covariation(**kw) == records
    stats = report.covariation_stats
    assert (stats['variants'], stats['dropped'], stats['pairs']) == (8, dropped, len(records))
    assert stats['columns'] == 8 + len({(r, p) for r, p, _c in kept}) and stats['native']['rows'] == len(ado.groups(text)[0])
    # fewer than two variants: no device call
    assert report.count_covariation(min_fraction=1.0, min_count=10 ** 9) == []
    assert report.covariation_stats == dict(variants=0, dropped=0, columns=0, pairs=0, native=None)


def test_chain_covariation_from_the_device_rows_and_from_the_file(tmp_path, monkeypatch):
    d = os.path.join(E2E_DIR, 'syn_pol')
    r1, r2 = os.path.join(d, 'R1.fastq.gz'), os.path.join(d, 'R2.fastq.gz')
    prelim, remap_csv, aligned = (tmp_path / n for n in ('prelim.csv', 'remap.csv', 'aligned.csv'))
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    with open(prelim) as f, open(remap_csv, 'w') as out, open(tmp_path / 'counts.csv', 'w') as cn:
        rm.remap(r1, r2, f, out, cn, gzip=True, work_path=str(tmp_path))
    with open(remap_csv) as f, open(aligned, 'w') as out:
        s2a.sam2aln(f, out)
    with open(aligned) as f:
        dev = _run(f, covariation_min_count=2)
    assert session.stats['aln2counts_source'] == 'device'
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    with open(aligned) as f:
        csv_way = _run(f, covariation_min_count=2)
    assert session.stats['aln2counts_source'] == 'csv'
    assert dev == csv_way
    assert dev['covariation'].count(os.linesep) > 1


# ---------------------------------------------------------------------------
# 4. two ranks
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_two_ranks_write_the_single_process_file(tmp_path):
    # the planted rows all lie in the second half of the file: the even rows
    # first, then the odd ones, puts them on both ranks' shares
    text, changed = _planted()
    head, *body = text.splitlines(keepends=True)
    text = head + ''.join(body[::2] + body[1::2])
    changed = sorted(i // 2 if i % 2 == 0 else (len(body) + 1) // 2 + i // 2 for i in changed)
    spec = dict(min_fraction=0.01, min_count=10, max_variants=256)
    root = tmp_path / 'cases'
    want = _run(io.StringIO(text))
    lines = co.expected(text)[0]
    assert want['covariation'] == _file(lines) and len(lines) == 4
    names = ('both_planted', 'rank0_planted')
    for name in names:
        os.makedirs(root / name)
        (root / name / 'aligned.csv').write_text(text)
        (root / name / 'covariation.json').write_text(json.dumps(spec))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, WORKER, '--cases', str(root)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    stats = [json.load(open(root / ('rank%d.json' % r))) for r in range(2)]
    for name in names:
        assert [s[name].get('mode') for s in stats] == ['sharded'] * 2, name
        n = [s[name]['rows'] for s in stats]
        assert min(n) >= 1 and max(n) < sum(n), (name, n)
        # planted rows on both ranks' shares
        assert changed[0] < n[0] <= changed[-1], (name, n)
        for k in PLAIN + ('covariation',):
            with open(root / name / (k + '.csv'), newline='') as f:
                assert f.read() == want[k], (name, k)

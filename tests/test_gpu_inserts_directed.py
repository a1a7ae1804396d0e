"""Directed cases for the insertion strings on the device (mh_a2c_inserts in
csrc/mh_a2c.hip: k_a2c_ins_hash / _verify / _gather around the shared
k_a2c_tab_count / k_a2c_tab_compact): rows loaded with a2c_load_rows, the
entries compared with a plain-Python restatement of the read loop of
InsertionWriter.write.  One test without a device pins the restatement to
the oracle's InsertionWriter (oracle/og_aln2counts.py Inserts) on the same
rows."""
import csv
import io
from collections import Counter

import pytest

import og_aln2counts as og
from micall_amd import aln2counts as a2c

SLOT = 2
# one codon per amino acid: a string of these translates letter for letter
CODON = dict(A='GCT', C='TGT', D='GAT', E='GAA', F='TTT', G='GGT', H='CAT', I='ATT', K='AAA',
             L='CTG', M='ATG', N='AAT', P='CCT', Q='CAA', R='CGT', S='TCT', T='ACT', V='GTT',
             W='TGG', Y='TAT')
LETTERS = sorted(CODON)


def _row(seq, offset=0, count=1):
    return dict(seq=seq, offset=offset, count=count)


def _nuc(aminos):
    return ''.join(CODON[a] for a in aminos)


def _word(i, n=3):
    """The i-th string of n amino acids (distinct for i < 20 ** n)."""
    return ''.join(LETTERS[(i // 20 ** k) % 20] for k in range(n))


def _piece(r, frame, left, right):
    """The slice 3 left - frame - offset .. min(3 right - frame - offset, len)
    of a row's seq, or None when it starts in the padding, is shorter than a
    codon or holds '-' or 'n'."""
    s = 3 * left - frame - r['offset']
    e = min(3 * right - frame - r['offset'], len(r['seq']))
    if s < 0 or e - s < 3:
        return None
    piece = r['seq'][s:e]
    return None if '-' in piece or 'n' in piece else piece


def keyed_pairs(rows, frame, ranges):
    """(range, row) pairs that produce a string: what the device sizes its
    table by (at least twice as many slots, 1024 at the least)."""
    return sum(_piece(r, frame, *rg) is not None for rg in ranges for r in rows)


def expected_inserts(rows, frame, ranges):
    """[(range index, count, first row, amino-acid string)] in (range, first
    row) order: per range (left, right) in codons and row, the whole codons
    of the row's slice translated and counted in row order."""
    out = []
    for k, (left, right) in enumerate(ranges):
        tally, first = Counter(), {}
        for i, r in enumerate(rows):
            piece = _piece(r, frame, left, right)
            if piece is None:
                continue
            aa = og.translate(piece[:len(piece) // 3 * 3])
            tally[aa] += r['count']
            first.setdefault(aa, i)
        out += sorted(((k, n, first[aa], aa) for aa, n in tally.items()), key=lambda t: t[2])
    return out


# ---------------------------------------------------------------------------
# the cases: name -> (rows, frame, ranges); rows carry the range [4, 7) at
# bases 12 .. 21 unless said otherwise
# ---------------------------------------------------------------------------
HEAD, TAIL = 'ACGTACGTACGT', 'TTGCA'
RANGE = [(4, 7)]


def _around(aminos, i=0, offset=0, count=1):
    """A row with `aminos` in codons 4 .. 7 and bases outside them that vary with i."""
    head = HEAD[:9] + 'ACGT'[i % 4] + 'ACGT'[i // 4 % 4] + 'ACGT'[i // 16 % 4]
    return _row((head + _nuc(aminos) + TAIL + 'ACGT'[i // 64 % 4])[offset:], offset, count)


def _framed(rows, frame):
    """The same rows read in `frame`: every row starts `frame` bases earlier."""
    return [_row(r['seq'], r['offset'] - frame, r['count']) if r['offset'] >= frame else
            _row(r['seq'][frame:], 0, r['count']) for r in rows]


def _build_cases():
    cases = {}
    cases['one_pair'] = ([_around('KLM')], 0, RANGE)
    # 256 and 257 (range, row) pairs: the last block is full / holds one pair
    cases['pairs_256'] = ([_around(_word(i % 7), i, count=i + 1) for i in range(128)], 0,
                          [(4, 7), (4, 6)])
    cases['pairs_257'] = ([_around(_word(i % 7), i, count=i + 1) for i in range(257)], 0, RANGE)
    # one string in every lane of every wave, different bases around it
    cases['wave_combining'] = ([_around('KLM', i, count=3 * i + 1) for i in range(200)], 0, RANGE)
    # six strings cycle through the 64 lanes of a wave: two are left to the
    # lane-by-lane remainder after the combining rounds
    six = [_around(_word(40 + i % 6), i, count=i + 1) for i in range(64)]
    for f in range(3):
        cases['six_keys_frame%d' % f] = (_framed(six, f), f, RANGE)
    # a string first seen in wave 0 (row 3) and again, with the larger count, in wave 1 (row 70)
    rows = [_around(_word(100 + i), i) for i in range(80)]
    rows[3] = _around('HHH', 3, count=2)
    rows[70] = _around('HHH', 70, count=900)
    cases['first_row_early_small'] = (rows, 0, RANGE)
    rows = list(rows)
    rows[3] = _around('HHH', 3, count=900)
    rows[70] = _around('HHH', 70, count=2)
    cases['first_row_early_large'] = (rows, 0, RANGE)
    # CTG / TTA / CTT are all L: one entry
    syn = [_row(HEAD + c + 'AAAATG' + TAIL, 0, n) for c, n in (('CTG', 5), ('TTA', 7), ('CTT', 11))]
    cases['synonymous'] = (syn + [_around('LKV', 9, count=13)], 0, RANGE)
    # rejected slices next to accepted ones
    good = HEAD + _nuc('KLM') + TAIL
    rej = [_row(good, 0, 1),
           _row(good[:14] + '-' + good[15:], 0, 2),        # '-' inside the range
           _row(good[:20] + 'n' + good[21:], 0, 4),        # 'n' inside the range
           _row(good[13:], 13, 8),                         # the range starts in the offset padding
           _row(good[12:], 12, 16),                        # starts exactly at the range
           _row(good[:12], 0, 32),                         # ends where the range starts
           _row(good[:14], 0, 64),                         # two bases of the range: no codon
           _row(good[:19], 0, 128),                        # two codons and a base: 'KL'
           _row(good[:11] + '-' + good[12:], 0, 256),      # '-' just before the range: accepted
           _row(good[:21] + 'n' + good[22:], 0, 512)]      # 'n' just after the range: accepted
    for f in range(3):
        cases['rejected_frame%d' % f] = (_framed(rej, f), f, RANGE)
    # three ranges, the middle one past every row's end
    three = [_around(_word(i % 5) + _word(i % 3), i, count=i + 1) for i in range(70)]
    cases['three_ranges'] = (three, 0, [(4, 6), (40, 45), (7, 10)])
    # the table is sized by the keyed pairs: 512 of them (500 distinct strings, 12 seen
    # twice) keep the 1024-slot minimum, just under half full; 640 (600 distinct) are the
    # first doubling to 2048
    for n, n_rows in ((500, 512), (600, 640)):
        cases['distinct_%d' % n] = ([_around(_word(i % n), i, count=i % 9 + 1)
                                     for i in range(n_rows)], 0, RANGE)
    # a sum past 2**32 cannot be loaded: a2c_load_rows refuses a group whose counts add up
    # to more than 2**32 - 1 (the codon counters are 32 bits), so the largest it takes:
    # the group's counts add up to 2**32 - 1, one string's to 2**32 - 8 (past 31 bits)
    cases['count_near_2_32'] = ([_around('KLM', 0, count=2 ** 31), _around('WWW', 1, count=7),
                                 _around('KLM', 2, count=2 ** 31 - 8)], 0, RANGE)
    return cases


CASES = _build_cases()
_EXPECTED = {}


def _expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = expected_inserts(*CASES[name])
    return _EXPECTED[name]


def test_cases_reach_what_they_are_for():
    def strings(name):
        return [e[3] for e in _expected(name)]
    assert _expected('one_pair') == [(0, 1, 0, 'KLM')]
    assert len(CASES['pairs_256'][0]) * len(CASES['pairs_256'][2]) == 256
    assert _expected('wave_combining') == [(0, sum(3 * i + 1 for i in range(200)), 0, 'KLM')]
    for f in range(3):
        assert len(_expected('six_keys_frame%d' % f)) == 6
        assert strings('rejected_frame%d' % f) == ['KLM', 'KL']
        assert [e[1] for e in _expected('rejected_frame%d' % f)] == [1 + 16 + 256 + 512, 128]
    assert (0, 902, 3, 'HHH') in _expected('first_row_early_small')
    assert (0, 902, 3, 'HHH') in _expected('first_row_early_large')
    assert _expected('synonymous') == [(0, 23, 0, 'LKM'), (0, 13, 3, 'LKV')]
    assert sorted({e[0] for e in _expected('three_ranges')}) == [0, 2]
    assert len(_expected('distinct_500')) == 500 and len(_expected('distinct_600')) == 600
    assert keyed_pairs(*CASES['distinct_500']) == 512      # 2 x 512 slots: the minimum table
    assert keyed_pairs(*CASES['distinct_600']) == 640      # more than 512: 2048 slots
    assert all(keyed_pairs(*CASES[name]) <= 512 for name in CASES if name != 'distinct_600')
    assert _expected('count_near_2_32')[0] == (0, 2 ** 32 - 8, 0, 'KLM')


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_is_the_oracles_insertion_writer(name):
    """The oracle's InsertionWriter over the same rows writes the
    restatement's entries (its ranges are runs of inserted codons, so of
    ranges that touch or overlap only the first is compared)."""
    rows, frame, ranges = CASES[name]
    if not all(a is b or a[1] < b[0] or b[1] < a[0] for a in ranges for b in ranges):
        ranges = ranges[:1]
    out = io.StringIO()
    w = og.Inserts(out)
    w.start_group('S', '15')
    for r in rows:
        w.add_nuc_read('-' * r['offset'] + r['seq'], r['count'])
    w.write({i for left, right in ranges for i in range(left, right)}, 'R', reading_frame=frame)
    got = [(int(left), aa, int(n)) for _, _, _, left, aa, n, _ in list(csv.reader(out.getvalue().splitlines()))[1:]]
    by_left = sorted(range(len(ranges)), key=lambda k: ranges[k][0])
    want = [(ranges[k][0] + 1, aa, n) for j in by_left
            for k, n, _, aa in expected_inserts(rows, frame, ranges) if k == j]
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_device_inserts(name):
    """The case's rows as the second group of the slot (after three rows of
    another): the entries, their summed counts and first rows are the
    restatement's, exactly."""
    from micall_amd import session
    rows, frame, ranges = CASES[name]
    ctx = session.context()
    lead = [_around('PPP', i) for i in range(3)]
    every = lead + rows
    ctx.a2c_load_rows(SLOT, [r['seq'] for r in every], [r['offset'] for r in every],
                      [r['count'] for r in every], [0, len(lead), len(every)], a2c._CODON_CHARS)
    got = ctx.a2c_inserts(SLOT, 1, frame, [r[0] for r in ranges], [r[1] for r in ranges])
    assert got == _expected(name)

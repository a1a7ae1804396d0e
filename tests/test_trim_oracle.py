"""The CPU statement of the 3' adapter trimming rules (tests/trim_oracle.py)
against the definition by brute force, the values the rules were checked on,
the order of the choice, and the arguments micall_amd.trim_fastqs refuses
(no GPU: the refusals come before the context is made)."""
import io
import random

import pytest

import trim_oracle
from micall_amd import trim_fastqs

NEXTERA = 'CTGTCTCTTATACACATCT'


def _edit_distance(a, b):
    """Plain unit-cost edit distance of two strings (Wagner-Fischer)."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        row = [i]
        for j in range(1, len(b) + 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])))
        prev = row
    return prev[-1]


def _brute(a, r, i, j):
    """(c(i, j), s(i, j)) by the definition: a[:i] against every r[s:j]."""
    dist = [_edit_distance(a[:i], r[s:j]) for s in range(j + 1)]
    c = min(dist)
    return c, dist.index(c)


def test_cost_and_origin_equal_the_definition():
    rng = random.Random(20)
    cases = 0
    for _ in range(360):
        a = ''.join(rng.choice('ACN') for _ in range(rng.randint(1, 6)))
        r = ''.join(rng.choice('ACN') for _ in range(rng.randint(0, 9)))
        cs = trim_oracle.cost_origin(a, r)
        rows = trim_oracle.table_rows(a, r)
        for i in range(len(a) + 1):
            for j in range(len(r) + 1):
                assert cs[i][j] == _brute(a, r, i, j), (a, r, i, j)
                assert (int(rows[i, j]) >> 16, int(rows[i, j]) & 0xffff) == cs[i][j], (a, r, i, j)
        cases += 1
    assert cases >= 300


def test_row_scan_equals_cell_recurrence_on_longer_reads():
    rng = random.Random(21)
    for _ in range(40):
        a = ''.join(rng.choice('ACGT') for _ in range(rng.randint(3, 64)))
        r = ''.join(rng.choice('ACGTN') for _ in range(rng.randint(0, 150)))
        if rng.random() < 0.5:
            r += a[:rng.randint(1, len(a))]
        assert trim_oracle.table_rows(a, r).tolist() == trim_oracle.table(a, r)


INSERT = ''.join(random.Random(100).choice('ACGT') for _ in range(100))
TAIL8 = 'GATTACAG'


def _kept(read, adapters=(NEXTERA,), min_overlap=3, rate=0.1):
    win = trim_oracle.best(read, list(adapters), min_overlap, trim_oracle.error_table(rate))
    return None if win is None else win[0]


def test_checked_values():
    E = trim_oracle.error_table(0.1)
    assert len(E) == 65 and E[19] == 1 and E[10] == 1 and E[9] == 0 and E[64] == 6
    assert E == trim_fastqs.error_table(0.1)
    assert len(INSERT) == 100
    assert _kept(INSERT + NEXTERA + TAIL8) == 100
    assert _kept(INSERT + NEXTERA[:9] + 'G' + NEXTERA[10:] + TAIL8) == 100    # one substitution
    assert _kept(INSERT + NEXTERA[:9] + NEXTERA[10:] + TAIL8) == 100          # one deleted base
    assert _kept(INSERT + NEXTERA[:9] + 'G' + NEXTERA[9:] + TAIL8) == 100     # one inserted base
    assert _kept(INSERT + NEXTERA[:10]) == 100
    assert _kept(INSERT + NEXTERA[:3]) == 100
    assert _kept(INSERT + NEXTERA[:2]) is None
    assert _kept(INSERT) is None
    # an N inside the occurrence is one error; two are one too many
    assert _kept(INSERT + NEXTERA[:5] + 'N' + NEXTERA[6:]) == 100
    assert _kept(INSERT + NEXTERA[:5] + 'NN' + NEXTERA[7:]) is None


def test_random_reads_lose_at_most_five_bases():
    """cutadapt's known behaviour at overlap 3: a random read ends in the
    adapter's first 3 to 5 bases about once in 48 (3000 * (1/64 + 1/256 +
    1/1024) = 61.5 expected); of these 3000, 70 do and none loses more."""
    rng = random.Random(13)
    lost = []
    for _ in range(3000):
        read = ''.join(rng.choice('ACGT') for _ in range(120))
        s = _kept(read)
        if s is not None:
            lost.append(120 - s)
    assert len(lost) == 70
    assert min(lost) == 3 and max(lost) == 5


def test_choice_order():
    E = trim_oracle.error_table(0.1)
    # equal origin and cost: the larger i wins over the lower adapter index
    assert trim_oracle.best('TTTTACGT', ['ACG', 'ACGT'], 3, E) == (4, 0, 4, 1)
    # equal origin: the smaller cost wins over the lower adapter index
    exact, off = 'ACGTTGCAAC', 'ACGTAGCAAC'
    assert trim_oracle.best('TTTT' + exact, [off, exact], 3, E) == (4, 0, 10, 1)
    assert trim_oracle.best('TTTT' + exact, [off], 3, E) == (4, 1, 10, 0)
    # equal origin, cost and i: the lower adapter index
    assert trim_oracle.best('TTTT' + exact, [exact, exact], 3, E) == (4, 0, 10, 0)
    # the smallest origin wins over everything: a one-error match further left
    assert trim_oracle.best('TT' + off + 'GG' + exact, [exact], 3, E) == (2, 1, 10, 0)
    # a partial match at the end, with the smallest origin among the prefixes
    assert trim_oracle.best('GGGGACGT', [exact], 3, E) == (4, 0, 4, 0)
    assert trim_oracle.best('GGGGACGT', [exact], 5, E) is None


def test_trim_bytes_by_direction_and_statistics():
    E = trim_oracle.error_table(0.1)
    data = (b'@M:1:F:1:1101:1:1 1:N:0:1\nGGGGACGTTGCAAC\n+\nABCDEFGHIJKLMN\n'
            b'@M:1:F:1:1101:1:1 2:N:0:1\nGGGGACGTTGCAAC\n+x\nABCDEFGHIJ\n'
            b'@M:1:F:1:1101:2:2 2:N:0:1\nGGTTTGGG\n+\nABCDEFGHIJ\n')
    out, stats = trim_oracle.trim_bytes(data, ['ACGTTGCAAC'], ['AAAA', 'TTTGGG'], 3, E)
    assert out == (b'@M:1:F:1:1101:1:1 1:N:0:1\nGGGG\n+\nABCD\n'
                   b'@M:1:F:1:1101:1:1 2:N:0:1\nGGGGACGTTGCAAC\n+x\nABCDEFGHIJ\n'
                   b'@M:1:F:1:1101:2:2 2:N:0:1\nGG\n+\nAB\n')
    assert stats == {(1, 0): [1, 10], (2, 1): [1, 6]}


def test_adapter_sets():
    assert trim_fastqs.resolve_adapters('nextera') == ([NEXTERA], [NEXTERA])
    assert trim_fastqs.resolve_adapters('truseq') == (['AGATCGGAAGAGCACACGTCTGAACTCCAGTCA'],
                                                      ['AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT'])
    assert trim_fastqs.resolve_adapters('truseq', 'nextera')[1] == [NEXTERA]
    assert trim_fastqs.resolve_adapters('ACGT') == (['ACGT'], ['ACGT'])
    assert trim_fastqs.resolve_adapters(['ACGT', 'GGG'], []) == (['ACGT', 'GGG'], [])


@pytest.mark.parametrize('adapters', [['AC'], ['A' * 65], ['ACGN'], ['acgt'], ['ACG'] * 9, 'nexterra', [b'ACGT']])
def test_adapters_refused(adapters):
    with pytest.raises(ValueError):
        trim_fastqs.resolve_adapters(adapters)
    with pytest.raises(ValueError):
        trim_fastqs.resolve_adapters('nextera', adapters)
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), adapters)
    if not isinstance(adapters, str) and all(isinstance(a, str) for a in adapters):
        with pytest.raises(ValueError):
            trim_oracle.check_args(adapters, [], 3, trim_oracle.error_table(0.1))


@pytest.mark.parametrize('kwargs', [dict(error_rate=1.0), dict(error_rate=-0.1), dict(error_rate=float('nan')),
                                    dict(min_overlap=0), dict(min_overlap=-3), dict(min_overlap=2.5)])
def test_rate_and_overlap_refused(kwargs):
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), 'nextera', **kwargs)


def test_oracle_refuses_what_the_library_refuses():
    E = trim_oracle.error_table(0.1)
    with pytest.raises(ValueError):
        trim_oracle.check_args(['ACGT'], ['ACGT'], 0, E)
    with pytest.raises(ValueError):
        trim_oracle.check_args(['ACGT'], ['ACGT'], 3, E[:64])
    with pytest.raises(ValueError):
        trim_oracle.check_args(['ACGT'], ['ACGT'], 3, [i for i in range(65)])   # rate 1
    with pytest.raises(ValueError):
        trim_oracle.best('A' * 65536, ['ACGT'], 3, E)

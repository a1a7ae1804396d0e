"""The CPU statement of the anchored 5' primer trimming rules
(tests/primer_oracle.py) against the definition by brute force, the values
the rules were checked on, the order of the choice, the false-match counts,
the make-up of the fuzz file, and the arguments micall_amd.trim_fastqs
refuses (no GPU: the refusals come before the context is made)."""
import io
import random

import pytest

import primer_cases
import primer_oracle
from micall_amd import trim_fastqs

P, INSERT, E = primer_cases.P, primer_cases.INSERT, primer_cases.E


def _edit_distance(a, b):
    """Plain unit-cost edit distance of two strings (Wagner-Fischer)."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        row = [i]
        for j in range(1, len(b) + 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])))
        prev = row
    return prev[-1]


def test_distances_equal_the_definition():
    rng = random.Random(40)
    for _ in range(300):
        p = ''.join(rng.choice('ACG') for _ in range(rng.randint(8, 14)))
        r = ''.join(rng.choice('ACGN') for _ in range(rng.randint(0, 20)))
        if rng.random() < 0.5:
            r = primer_cases._edited(rng, p, rng.randint(0, 3)) + r
        max_err = rng.randint(0, 4)
        got = primer_oracle.distances(p, r, max_err)
        assert len(got) == min(len(r), len(p) + max_err) + 1
        assert got == [_edit_distance(p, r[:j]) for j in range(len(got))], (p, r)


def test_array_form_equals_cell_recurrence():
    rng = random.Random(41)
    for _ in range(60):
        primers = [''.join(rng.choice('ACGT') for _ in range(rng.randint(8, 64))) for _ in range(rng.randint(1, 7))]
        r = ''.join(rng.choice('ACGTN') for _ in range(rng.randint(0, 90)))
        if rng.random() < 0.6:
            r = primer_cases._edited(rng, rng.choice(primers), rng.randint(0, 4)) + r
        table = primer_oracle.error_table(rng.choice([0.0, 0.1, 0.25]))
        assert primer_oracle.distances_many(primers, r, table) == \
            [primer_oracle.distances(p, r, table[len(p)]) for p in primers]
    assert primer_oracle.distances_many([], 'ACGT', E) == []


def _bit_vector_columns(p, r, cols):
    """[D(j) for j in 0..cols] by the 64-bit word operations of k_primer:
    Myers' vertical deltas pv / mv over the primer's rows, with the horizontal
    delta shifted into row 0 set to +1 (D[0][j] = j)."""
    m, word = len(p), (1 << 64) - 1
    eq = {c: sum(1 << i for i, b in enumerate(p) if b == c) for c in 'ACGT'}
    pv, mv, score, top, out = word, 0, m, 1 << (m - 1), [m]
    for j in range(cols):
        e = eq.get(r[j], 0)
        xv = e | mv
        xh = ((((e & pv) + pv) & word) ^ pv) | e
        ph = (mv | ~(xh | pv)) & word
        mh = pv & xh
        score += (1 if ph & top else 0) - (1 if mh & top else 0)
        ph = (ph << 1 | 1) & word
        mh = (mh << 1) & word
        pv = (mh | ~(xv | ph)) & word
        mv = ph & xv
        out.append(score)
    return out


def test_bit_vector_columns_equal_the_recurrence():
    """The kernel's formulation, restated on Python integers: the boundary
    that makes it a distance from the read's start and not a search."""
    rng = random.Random(42)
    pairs = 0
    for _ in range(300):
        primers = [''.join(rng.choice('ACGT') for _ in range(rng.choice([8, 9, 31, 32, 33, 63, 64])))
                   for _ in range(4)]
        r = ''.join(rng.choice('ACGTN') for _ in range(rng.randint(0, 90)))
        if rng.random() < 0.6:
            r = primer_cases._edited(rng, rng.choice(primers), rng.randint(0, 5)) + r
        for p in primers:
            want = primer_oracle.distances(p, r, E[len(p)])
            assert _bit_vector_columns(p, r, len(want) - 1) == want, (p, r)
            pairs += 1
    assert pairs == 1200


def test_checked_values():
    assert len(E) == 65 and E[22] == 2 and E[8] == 0 and E[64] == 6
    assert E == trim_fastqs.error_table(0.1)
    assert len(P) == 22 and len(INSERT) == 70
    for name, read, lead, cost in primer_cases.LITERALS:
        win = primer_oracle.best(read, [P], E)
        assert win == (None if lead is None else (lead, cost, 0)), name
    # the record cut to nothing stays, as an empty record
    data = primer_cases.record(0, 1, P).encode()
    assert primer_oracle.trim_bytes(data, [P], [P], E)[0].split(b'\n')[1:4] == [b'', b'+', b'']


def test_choice_order():
    read = P + INSERT
    # the larger m - D wins over the lower index
    assert primer_oracle.best(read, [P[:12], P], E) == (22, 0, 1)
    assert primer_oracle.best(read, [P, P], E) == (22, 0, 0)
    # equal m - D: the smaller D wins (21 bases exact over 22 bases with one error)
    assert primer_oracle.best(P[:21] + 'TGGAT', [P, P[:21]], E) == (21, 0, 1)
    assert primer_oracle.best(P[:21] + 'TGGAT', [P], E) == (22, 1, 0)
    # equal m - D and D: the larger j (the primer's last base deleted, or replaced by the next read base)
    cut = P[:21] + 'GGGAT'
    assert primer_oracle.distances(P, cut, 2)[21:24] == [1, 1, 2]
    assert primer_oracle.best(cut, [P], E) == (22, 1, 0)
    # equal m - D, D and j: the lower index
    assert primer_oracle.best(read, ['A' * 22, P, P], E) == (22, 0, 1)


def test_false_matches():
    """1000 random 100-mers against 200 random primers: none of length 12,
    16, 20 or 30 matches, of length 8 (E = 0, 200 / 4**8 expected per read,
    3.05 in all) 3 do."""
    def count(m):
        rng = random.Random(66)
        primers = [primer_cases._bases(rng, m) for _ in range(200)]
        reads = [primer_cases._bases(rng, 100) for _ in range(1000)]
        return sum(primer_oracle.best(r, primers, E) is not None for r in reads)
    assert [count(m) for m in (12, 16, 20, 30)] == [0, 0, 0, 0]
    assert count(8) == 3


def test_trim_bytes_by_direction_and_statistics():
    a, b = 'ACGTTGCAAC', 'TTTGGGCC'
    data = (b'@M:1:F:1:1101:1:1 1:N:0:1\nACGTTGCAACGGGG\n+\nABCDEFGHIJKLMN\n'
            b'@M:1:F:1:1101:1:1 2:N:0:1\nACGTTGCAACGGGG\n+x\nABCDEFGHIJ\n'
            b'@M:1:F:1:1101:2:2 2:N:0:1\nTTTGGGCCAT\n+\nABCDE\n'
            b'@M:1:F:1:1101:3:3 1:N:0:1\nACGTAGCAACGGGG\n+\nABCDEFGHIJKLMNOP\n')
    out, stats = primer_oracle.trim_bytes(data, [a], ['AAAAAAAA', b], E)
    assert out == (b'@M:1:F:1:1101:1:1 1:N:0:1\nGGGG\n+\nKLMN\n'
                   b'@M:1:F:1:1101:1:1 2:N:0:1\nACGTTGCAACGGGG\n+x\nABCDEFGHIJ\n'
                   b'@M:1:F:1:1101:2:2 2:N:0:1\nAT\n+\n\n'
                   b'@M:1:F:1:1101:3:3 1:N:0:1\nGGGG\n+\nKLMNOP\n')
    assert stats == {(1, 0): [2, 20], (2, 1): [1, 8]}


def test_fuzz_file_make_up():
    lists = primer_cases.fuzz_primers()
    assert [len(x) for x in lists] == [96, 96] and lists[0] != lists[1]
    assert all(18 <= len(p) <= 30 for x in lists for p in x)
    heads = primer_cases.fuzz_fastq().split(b'\n')[0::4]
    assert sum(b' 1:' in h for h in heads) == sum(b' 2:' in h for h in heads) == 2000
    _, stats, _, _, classes = primer_cases.fuzz_expected()
    records = sum(classes.values())
    assert 3900 <= records <= 4100 and set(classes) == {'exact', 'errors', 'untrimmed'}
    assert all(5 * v >= records for v in classes.values()), classes
    assert {d for d, _ in stats} == {1, 2}


def test_directed_file_make_up():
    """The shapes tests/test_gpu_primers.py relies on are in the file: every
    lane round wins, index 3 wins over its copy at 200, a lead of 70."""
    want, stats, _, _ = primer_cases.directed_expected()
    assert {k for d, k in stats if d == 1} == {0, 3, 5, 63, 64, 255} and (2, 0) in stats
    lost = [len(a) - len(b) for a, b in zip(primer_cases.directed_fastq().split(b'\n')[1::4],
                                           want.split(b'\n')[1::4])]
    assert max(lost) == 70 and 8 in lost and 0 in lost


def test_resolve_primers(tmp_path):
    assert trim_fastqs.resolve_primers(None) == ([], [])
    assert trim_fastqs.resolve_primers([P]) == ([('primer1', P)], [('primer1', P)])
    assert trim_fastqs.resolve_primers({'left': P}, [P[:8], P]) == \
        ([('left', P)], [('primer1', P[:8]), ('primer2', P)])
    assert trim_fastqs.resolve_primers([P], []) == ([('primer1', P)], [])
    fasta = tmp_path / 'scheme.fasta'
    fasta.write_text('>nCoV_1_LEFT pool 1\n{}\n{}\n\n>nCoV_1_RIGHT\n{}\n'.format(P[:10], P[10:], P[:18]))
    assert trim_fastqs.resolve_primers(str(fasta)) == ([('nCoV_1_LEFT', P), ('nCoV_1_RIGHT', P[:18])],) * 2
    assert trim_fastqs.resolve_primers(fasta, None)[0][0] == ('nCoV_1_LEFT', P)


@pytest.mark.parametrize('primers', [['ACGTACGT'] * 257, ['ACGTACG'], ['A' * 65], [P[:10] + 'R' + P[11:]],
                                     [P.lower()], [P.encode()]])
def test_primers_refused(primers):
    with pytest.raises(ValueError):
        trim_fastqs.resolve_primers(primers)
    with pytest.raises(ValueError):
        trim_fastqs.resolve_primers([P], primers)
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers1=primers)
    if all(isinstance(p, str) for p in primers):
        with pytest.raises(ValueError):
            primer_oracle.check_args(primers, [], E)


def test_refused_primer_is_named(tmp_path):
    bad = P[:10] + 'R' + P[11:]
    with pytest.raises(ValueError, match='HCV_7_LEFT.*' + bad):
        trim_fastqs.resolve_primers({'HCV_6_LEFT': P, 'HCV_7_LEFT': bad})
    fasta = tmp_path / 'twice.fasta'
    fasta.write_text('>a\n{}\n>b\n{}\n>a\n{}\n'.format(P, P, P))
    with pytest.raises(ValueError, match="'a' is given twice"):
        trim_fastqs.resolve_primers(str(fasta))
    with pytest.raises(ValueError, match="'a' is given twice"):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers1=str(fasta))
    # a string is a file's name, never a sequence
    with pytest.raises(ValueError, match='no such FASTA file'):
        trim_fastqs.resolve_primers(P)


@pytest.mark.parametrize('rate', [1, 1.0, -0.1, float('nan')])
def test_rate_refused(rate):
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers1=[P], primer_error_rate=rate)


def test_oracle_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        primer_oracle.check_args([P], [P], E[:64])
    with pytest.raises(ValueError):
        primer_oracle.check_args([P], [P], list(range(65)))          # rate 1: E[m] >= m
    with pytest.raises(ValueError):
        primer_oracle.check_args([P], [P], [0] * 64 + [64])          # 64 + 64 > 127
    primer_oracle.check_args([P] * 256, [], primer_oracle.error_table(0.98))

"""The CPU statement of the 3' primer trimming rules (tests/primer3_oracle.py)
against the definitions by brute force, the word operations of k_primer3
against the cell recurrences, the array form against the plain one, the
values the rules were checked on, the order of the choice, the false-match
counts, the make-up of the test files, 'mates' and the arguments
micall_amd.trim_fastqs refuses (no GPU: the refusals come before the context
is made)."""
import io
import random

import pytest

import primer3_cases
import primer3_oracle
import primer_cases
from micall_amd import trim_fastqs

P, INSERT, E, MIN_OVERLAP = primer3_cases.P, primer3_cases.INSERT, primer3_cases.E, primer3_cases.MIN_OVERLAP


def _edit_distance(a, b):
    """Plain unit-cost edit distance of two strings (Wagner-Fischer)."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        row = [i]
        for j in range(1, len(b) + 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])))
        prev = row
    return prev[-1]


def _random_case(rng, lo=8, hi=14):
    """(primer, text): random, or with a mutated copy of the primer planted,
    or ending inside the primer."""
    p = ''.join(rng.choice('ACG') for _ in range(rng.randint(lo, hi)))
    x = ''.join(rng.choice('ACGN') for _ in range(rng.randint(0, 20)))
    kind = rng.random()
    if kind < 0.35:
        x += primer_cases._edited(rng, p, rng.randint(0, 3)) + 'GATT'[:rng.randint(0, 4)]
    elif kind < 0.7:
        x += primer_cases._edited(rng, p[:rng.randint(3, len(p) - 1)], rng.randint(0, 2))
    return p, x


def test_tables_equal_the_definitions():
    """F(b) = min over e of ed(p, r[n-b:e]); G(b) = min over i of
    ed(p[:i], r[n-b:n])."""
    rng = random.Random(50)
    for _ in range(300):
        p, x = _random_case(rng)
        n = len(x)
        assert primer3_oracle.full_costs(p, x) == \
            [min(_edit_distance(p, x[n - b:e]) for e in range(n - b, n + 1)) for b in range(n + 1)], (p, x)
        assert primer3_oracle.partial_costs(p, x) == \
            [min(_edit_distance(p[:i], x[n - b:]) for i in range(len(p) + 1)) for b in range(n + 1)], (p, x)


def _bit_vector_columns(p, x, search):
    """[A[m][b]] (search) or [B[m][b]] for b in 0 ..= len(x) by the 64-bit
    word operations of k_primer3 on the reversed primer, the text taken from
    its end: Myers' vertical deltas pv / mv, for A from pv = ~0, mv = 0,
    score m with a horizontal delta of 0 shifted into row 0, for B from
    pv = mv = 0, score 0 with +1 shifted in."""
    m, word = len(p), (1 << 64) - 1
    eq = {c: sum(1 << i for i, b in enumerate(p[::-1]) if b == c) for c in 'ACGT'}
    pv, mv, score = (word, 0, m) if search else (0, 0, 0)
    top, out = 1 << (m - 1), [score]
    for c in x[::-1]:
        e = eq.get(c, 0)
        xv = e | mv
        xh = ((((e & pv) + pv) & word) ^ pv) | e
        ph = (mv | ~(xh | pv)) & word
        mh = pv & xh
        score += (1 if ph & top else 0) - (1 if mh & top else 0)
        ph = (ph << 1 | (0 if search else 1)) & word
        mh = (mh << 1) & word
        pv = (mh | ~(xv | ph)) & word
        mv = ph & xv
        out.append(score)
    return out


def test_bit_vector_columns_equal_both_recurrences():
    rng = random.Random(51)
    pairs = 0
    for _ in range(120):
        primers = [''.join(rng.choice('ACGT') for _ in range(m)) for m in (8, 31, 32, 33, 63, 64)]
        x = ''.join(rng.choice('ACGTN') for _ in range(rng.randint(0, 90)))
        pick = rng.choice(primers)
        kind = rng.random()
        if kind < 0.4:
            x += primer_cases._edited(rng, pick, rng.randint(0, 5)) + 'GATTACA'[:rng.randint(0, 7)]
        elif kind < 0.7:
            x += primer_cases._edited(rng, pick[:rng.randint(4, len(pick) - 1)], rng.randint(0, 3))
        for p in primers:
            assert _bit_vector_columns(p, x, True) == primer3_oracle.full_costs(p, x), (p, x)
            assert _bit_vector_columns(p, x, False) == primer3_oracle.partial_costs(p, x), (p, x)
            pairs += 1
    assert pairs == 720


def test_array_form_equals_the_plain_one():
    rng = random.Random(52)
    trimmed = 0
    for _ in range(40):
        primers = [''.join(rng.choice('ACGT') for _ in range(rng.choice([8, 9, 18, 22, 30, 33, 63, 64])))
                   for _ in range(rng.randint(1, 6))]
        reads, leads = [], []
        for _ in range(8):
            pick = rng.choice(primers)
            r = ''.join(rng.choice('ACGTN') for _ in range(rng.randint(0, 100)))
            kind = rng.random()
            if kind < 0.35:
                r += primer_cases._edited(rng, pick, rng.randint(0, 4)) + 'GATTACA'[:rng.randint(0, 7)]
            elif kind < 0.7:
                r += primer_cases._edited(rng, pick[:rng.randint(3, len(pick) - 1)], rng.randint(0, 2))
            reads.append(r)
            leads.append(rng.choice([0, 0, rng.randint(0, len(r))]))
        table = primer3_oracle.error_table(rng.choice([0.0, 0.1, 0.25]))
        min_overlap = rng.choice([1, 3, 12, 20, 64])
        want = [primer3_oracle.best(r, lead, primers, table, min_overlap) for r, lead in zip(reads, leads)]
        assert primer3_oracle.best_many(reads, leads, primers, table, min_overlap) == want
        trimmed += sum(w is not None for w in want)
    assert trimmed > 100
    assert primer3_oracle.best_many(['ACGT'], [0], [], E, 12) == [None]
    assert primer3_oracle.best_many([], [], [P], E, 12) == []


def test_checked_values():
    assert len(E) == 65 and E[22] == 2 and E[12:20] == [1] * 8 and E[10] == 1 and E[9] == 0
    assert E == trim_fastqs.error_table(0.1)
    assert len(P) == 22 and len(INSERT) == 70 and not set(INSERT) - set('ACGT')
    for name, read, cut, cost, kind in primer3_cases.LITERALS:
        win = primer3_oracle.best(read, 0, [P], E, MIN_OVERLAP)
        assert win == (None if cut is None else (cut, cost, 0, kind)), name
        assert primer3_oracle.best_many([read], [0], [P], E, MIN_OVERLAP) == [win], name
    # the record cut to nothing stays, as an empty record
    data = primer3_cases.record(0, 1, P).encode()
    assert primer3_oracle.trim_bytes(data, None, [P], [P], E, MIN_OVERLAP)[0].split(b'\n')[1:4] == [b'', b'+', b'']


def test_choice_order():
    best = primer3_oracle.best
    read = INSERT + P
    # the larger L - D wins over the lower index
    assert best(read, 0, [P[8:], P], E, MIN_OVERLAP) == (22, 0, 1, 'full')
    assert best(read, 0, [P, P], E, MIN_OVERLAP) == (22, 0, 0, 'full')
    # equal L - D: the smaller D wins, a full candidate or a partial one
    lists = primer3_cases.directed_primers()[1]
    a, c, a2, c2 = lists[:4]
    assert best('TTTT' + 'G' + a, 0, [c, a], E, MIN_OVERLAP) == (13, 0, 1, 'full')
    assert best('TTTT' + 'G' + a, 0, [c], E, MIN_OVERLAP) == (14, 1, 0, 'partial')
    swapped = a2[:10] + c2[9] + a2[11:]
    assert best('TTTT' + swapped, 0, [a2, c2], E, MIN_OVERLAP) == (20, 0, 1, 'partial')
    assert best('TTTT' + swapped, 0, [a2], E, MIN_OVERLAP) == (21, 1, 0, 'full')
    # equal L - D and D: the larger b (the primer's first base missing, or replaced by the read's base there)
    assert primer3_oracle.full_costs(P, 'GGGGT' + P[1:])[21:24] == [1, 1, 2]
    assert best('GGGGT' + P[1:], 0, [P], E, MIN_OVERLAP) == (22, 1, 0, 'full')
    # nothing in front of the lead is searched, and a cut never falls before it
    assert best(read, 70, [P], E, MIN_OVERLAP) == (22, 0, 0, 'full')
    assert best(read, 71, [P], E, MIN_OVERLAP) == (21, 1, 0, 'full')
    assert best(read, 73, [P], E, MIN_OVERLAP) is None
    assert best(read, len(read), [P], E, MIN_OVERLAP) is None
    # below min_overlap no partial match
    assert best(INSERT + P[:12], 0, [P], E, 13) == (13, 1, 0, 'partial')     # with the insert's last base
    assert best(INSERT + P[:12], 0, [P], E, 14) is None


def test_false_matches():
    """300 random 150-mers against 200 random primers of 18 to 30 bases: none
    is trimmed at min_overlap 12 (the default), some are at 8 and 10, where
    E[10] = 1 lets 9 of 10 bases pass."""
    rng = random.Random(67)
    primers = [primer_cases._bases(rng, rng.randint(18, 30)) for _ in range(200)]
    reads = [primer_cases._bases(rng, 150) for _ in range(300)]

    def count(min_overlap):
        return sum(w is not None for w in primer3_oracle.best_many(reads, [0] * 300, primers, E, min_overlap))
    assert [count(v) for v in (12, 10, 8)] == [0, 1, 2]


def test_trim_bytes_by_direction_and_statistics():
    a, b = 'ACGTTGCAAC', 'TTTGGGCC'
    data = (b'@M:1:F:1:1101:1:1 1:N:0:1\nGGGGACGTTGCAAC\n+\nABCDEFGHIJKLMN\n'
            b'@M:1:F:1:1101:1:1 2:N:0:1\nGGGGACGTTGCAAC\n+x\nABCDEF\n'
            b'@M:1:F:1:1101:2:2 2:N:0:1\nATTTTGGGCC\n+\nABC\n'
            b'@M:1:F:1:1101:3:3 1:N:0:1\nGGGGACGTTGCAACTT\n+\nABCDEFGHIJKLMNOPQR\n')
    out, stats = primer3_oracle.trim_bytes(data, None, [a], ['AAAAAAAA', b], E, 8)
    assert out == (b'@M:1:F:1:1101:1:1 1:N:0:1\nGGGG\n+\nABCD\n'
                   b'@M:1:F:1:1101:1:1 2:N:0:1\nGGGGACGTTGCAAC\n+x\nABCDEF\n'
                   b'@M:1:F:1:1101:2:2 2:N:0:1\nAT\n+\nAB\n'
                   b'@M:1:F:1:1101:3:3 1:N:0:1\nGGGG\n+\nABCD\n')
    assert stats == {(1, 0): [2, 22], (2, 1): [1, 8]}
    # with leads: the front goes as the 5' pass decided, the end as the 3' pass does
    out, stats = primer3_oracle.trim_bytes(data, [2, 0, 1, 3], [a], ['AAAAAAAA', b], E, 8)
    assert out.split(b'\n')[1::4] == [b'GG', b'GGGGACGTTGCAAC', b'T', b'G']
    assert out.split(b'\n')[3::4] == [b'CD', b'ABCDEF', b'B', b'D']
    assert stats == {(1, 0): [2, 22], (2, 1): [1, 8]}


def test_fuzz_file_make_up():
    lists = primer3_cases.fuzz_primers()
    assert [len(x) for x in lists] == [96, 96] and lists[0] != lists[1]
    assert all(18 <= len(p) <= 30 for x in lists for p in x)
    lines = primer3_cases.fuzz_fastq().split(b'\n')
    assert sum(b' 1:' in h for h in lines[0::4]) == sum(b' 2:' in h for h in lines[0::4]) == 2000
    assert all(60 <= len(s) <= 160 for s in lines[1:-1:4])
    _, stats, _, _, classes = primer3_cases.fuzz_expected()
    records = sum(classes.values())
    assert 3900 <= records <= 4100 and set(classes) == {'full exact', 'full errors', 'partial', 'untrimmed'}
    assert all(10 * v >= records for v in classes.values()), classes
    assert {d for d, _ in stats} == {1, 2}


def test_directed_file_make_up():
    """The shapes tests/test_gpu_primers3.py relies on are in the file:
    every lane round wins, index 3 wins over its copy at 200, a partial match
    of 63 bases, cuts on both sides of the block boundaries, every class."""
    want, stats, _, _, classes = primer3_cases.directed_expected()
    assert {k for d, k in stats if d == 1} == set(primer3_cases.WINNERS)
    assert {k for d, k in stats if d == 2} == {0, 3, 4}
    assert set(classes) == {'full exact', 'full errors', 'partial', 'untrimmed'}
    src = primer3_cases.directed_fastq().split(b'\n')[1::4]
    cut = [len(a) - len(b) for a, b in zip(src, want.split(b'\n')[1::4])]
    assert {0, 8, MIN_OVERLAP, 63, 64} <= set(cut)
    assert any(64 < b < 64 + 30 for b in cut) and any(128 < b < 128 + 64 for b in cut)
    assert {len(s) for s in src} >= set(primer3_cases.TEXT_LENGTHS)
    # the 63 bases of the 64-base primer, behind an insert and alone; the two tie pairs
    assert cut[-4:] == [63, 63, 13, 20]


def test_lead_file_make_up():
    out, stats5, stats3, leads, cuts = primer3_cases.lead_expected()
    assert leads == [22] * 9
    assert cuts == [22, 26, 21, 0, 0, 13, 0, 22, 0]
    assert out.split(b'\n')[1::4][:7] == [b'', b'', b'', primer3_cases.Q9[1:].encode(),
                                          (primer3_cases.Q9[1:] + 'ACCA').encode(), b'', b'']
    assert stats5 == {(1, 0): [5, 110], (2, 0): [4, 88]}
    assert stats3 == {(1, 0): [1, 22], (1, 1): [1, 21], (2, 0): [3, 61]}


def test_chain_file_make_up():
    out, astats, stats5, stats3, _, _ = primer3_cases.chain_expected()
    assert sum(v[0] for v in astats.values()) > 100
    assert sum(v[0] for v in stats5.values()) > 400
    assert sum(v[0] for v in stats3.values()) > 200
    assert {d for d, _ in stats3} == {1, 2} and len(stats3) == 4


def test_mates():
    rc = trim_fastqs.reverse_complement
    assert rc('AACGT') == 'ACGTT' == primer3_cases.reverse_complement('AACGT')
    five = trim_fastqs.resolve_primers({'f1': P, 'f2': P[:18]}, [P[2:], P[:9]])
    got = trim_fastqs.resolve_primers3('mates', 'mates', five)
    assert got == ([('primer1', rc(P[2:])), ('primer2', rc(P[:9]))], [('f1', rc(P)), ('f2', rc(P[:18]))])
    # explicit sequences are taken as they read in the read; no side defaults to the other
    assert trim_fastqs.resolve_primers3([P], None, five) == ([('primer1', P)], [])
    assert trim_fastqs.resolve_primers3(None, {'x': P}, ([], [])) == ([], [('x', P)])
    assert trim_fastqs.resolve_primers3(None, None, five) == ([], [])
    assert trim_fastqs.resolve_primers3('mates', None, five)[1] == []
    with pytest.raises(ValueError, match="primers3_1 is 'mates' and primers2 is empty"):
        trim_fastqs.resolve_primers3('mates', None, trim_fastqs.resolve_primers([P], []))
    with pytest.raises(ValueError, match="primers3_2 is 'mates' and primers1 is empty"):
        trim_fastqs.resolve_primers3(None, 'mates', ([], [('a', P)]))
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_1='mates')


def test_mates_from_fasta(tmp_path):
    fasta = tmp_path / 'scheme.fasta'
    fasta.write_text('>nCoV_1_RIGHT\n{}\n'.format(P))
    assert trim_fastqs.resolve_primers3(str(fasta), None, ([], [])) == ([('nCoV_1_RIGHT', P)], [])


@pytest.mark.parametrize('primers', [['ACGTACGT'] * 257, ['ACGTACG'], ['A' * 65], [P[:10] + 'R' + P[11:]],
                                     [P.lower()], [P.encode()]])
def test_primers3_refused(primers):
    with pytest.raises(ValueError):
        trim_fastqs.resolve_primers3(primers, None, ([], []))
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_1=primers)
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_2=primers)
    if all(isinstance(p, str) for p in primers):
        with pytest.raises(ValueError):
            primer3_oracle.check_args(primers, [], E, MIN_OVERLAP)


def test_refused_primer3_is_named():
    bad = P[:10] + 'R' + P[11:]
    with pytest.raises(ValueError, match='HCV_7_RIGHT.*' + bad):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_2={'HCV_6_RIGHT': P, 'HCV_7_RIGHT': bad})
    # a string that is not 'mates' is a file's name, never a sequence
    with pytest.raises(ValueError, match='no such FASTA file'):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_1=P)


@pytest.mark.parametrize('min_overlap', [0, 65, -1, 12.5, True])
def test_min_overlap_refused(min_overlap):
    with pytest.raises(ValueError, match='primer3_min_overlap'):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_1=[P], primer3_min_overlap=min_overlap)
    if min_overlap is not True:
        with pytest.raises(ValueError):
            primer3_oracle.check_args([P], [], E, min_overlap)


@pytest.mark.parametrize('rate', [1, 1.0, -0.1, float('nan')])
def test_rate_refused(rate):
    with pytest.raises(ValueError):
        trim_fastqs.trim(io.BytesIO(), io.BytesIO(), (), primers3_1=[P], primer_error_rate=rate)


def test_oracle_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        primer3_oracle.check_args([P], [P], E[:64], MIN_OVERLAP)
    with pytest.raises(ValueError):
        primer3_oracle.check_args([P], [P], list(range(65)), MIN_OVERLAP)      # rate 1: E[m] >= m
    primer3_oracle.check_args([P] * 256, [], primer3_oracle.error_table(0.98), 64)

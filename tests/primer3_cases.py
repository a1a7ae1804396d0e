"""Inputs shared by tests/test_primer3_oracle.py, tests/test_gpu_primers3.py and
tests/test_gpu_shard_primers3.py: the literal cases the rules were checked
on, the directed records, the fuzz FASTQ and the chain file for 3' primer
trimming, each with what tests/primer3_oracle.py makes of it after
oracle/og_censor.py (and tests/trim_oracle.py and tests/primer_oracle.py,
where adapters and 5' primers are set), computed once per process."""
import functools
import random

import og_censor
import primer3_oracle
import primer_cases
import primer_oracle
import trim_cases
import trim_oracle
from trim_cases import _bases, record

E = primer3_oracle.error_table(0.1)
MIN_OVERLAP = 12
P = 'ACGTTGCATGCCAGTAGGATCC'                          # 22 bases, E[22] = 2, E[12..19] = 1
INSERT = _bases(random.Random(303), 70)
P5 = primer_cases.P                                   # a 5' primer, 22 bases

_COMPLEMENT = str.maketrans('ACGT', 'TGCA')


def reverse_complement(seq):
    return seq.translate(_COMPLEMENT)[::-1]


# (name, read, bases cut or None, cost, kind): the values the rules were
# checked on, the 3' list being [P] at rate 0.1 and min_overlap 12
LITERALS = [
    ('primer then six bases', INSERT + P + 'GGAACC', 28, 0, 'full'),
    ('primer at the end', INSERT + P, 22, 0, 'full'),
    ('one base N, then TT', INSERT + P[:9] + 'N' + P[10:] + 'TT', 24, 1, 'full'),
    ('one base deleted, then TT', INSERT + P[:9] + P[10:] + 'TT', 23, 1, 'full'),
    ('one base inserted, then TT', INSERT + P[:9] + 'A' + P[9:] + 'TT', 25, 1, 'full'),
    ('three bases N', INSERT + P[:4] + 'N' + P[5:10] + 'N' + P[11:16] + 'N' + P[17:], None, None, None),
    ('first 12 bases', INSERT + P[:12], 12, 0, 'partial'),
    ('first 11 bases', INSERT + P[:11], 12, 1, 'partial'),     # the insert's last base is taken along
    ('first 14 bases, one N', INSERT + P[:6] + 'N' + P[7:14], 14, 1, 'partial'),
    ('primer alone', P, 22, 0, 'full'),
    ('empty', '', None, None, None),
]


def literals_fastq():
    return ''.join(record(i, 1 + i % 2, read) for i, (_, read, _, _, _) in enumerate(LITERALS)).encode()


def stats_of(result):
    """trim()'s returned 3' primer rows in the oracle's form: {(direction,
    primer index): [reads, bases]} without the primers that won nothing."""
    out, seen = {}, {}
    for row in result['primers3']:
        k = seen.get(row['direction'], 0)
        seen[row['direction']] = k + 1
        if row['reads'] or row['bases']:
            out[(row['direction'], k)] = [row['reads'], row['bases']]
    return out


def _edited(rng, p, edits):
    return primer_cases._edited(rng, p, edits)


# ---- the directed records --------------------------------------------------
TEXT_LENGTHS = (0, 1, MIN_OVERLAP - 1, MIN_OVERLAP, 63, 64, 65, 127, 128, 129, 300)
WINNERS = (0, 3, 5, 63, 64, 130, 255)      # every lane round of the kernel: 0-63, 64-127, 128-191, 192-255


@functools.lru_cache(maxsize=None)
def directed_primers():
    """(3' list 1, 3' list 2).  List 1: 256 primers of 18 to 30 bases, but
    index 0 of 8 bases, index 5 of 64, and index 200 a copy of index 3.  List
    2 (the two candidates of each pair tie on L - D): a of 13 bases and c
    whose first 14 are a base and a with one base replaced; a2 of 21 bases
    and c2 whose first 20 are a2[1:] with one base replaced -- so a2 with
    that base replaced is a full match of cost 1 and a partial match of c2
    of cost 0; then one primer of 64 bases."""
    rng = random.Random(187)
    one = [_bases(rng, rng.randint(18, 30)) for _ in range(256)]
    one[0] = _bases(rng, 8)
    one[5] = _bases(rng, 64)
    one[200] = one[3]
    a = _bases(rng, 13)
    c = 'G' + a[:6] + ('A' if a[6] != 'A' else 'C') + a[7:] + _bases(rng, 10)
    a2 = _bases(rng, 21)
    swapped = a2[:10] + ('A' if a2[10] != 'A' else 'C') + a2[11:]
    c2 = swapped[1:] + _bases(rng, 8)
    return one, [a, c, a2, c2, _bases(rng, 64)]


@functools.lru_cache(maxsize=None)
def directed_fastq():
    """For the primers WINNERS of list 1 and the 64-base one of list 2: the
    primer behind an insert with and without a tail, with one edit of each
    kind, an N and a lower-case base inside it, cut to a prefix at the read's
    end, ending exactly in column 64 and straddling columns 64 | 65 and
    128 | 129 of the backward scan, reads of TEXT_LENGTHS bases that end in
    the primer, quality lines shorter and longer than the sequence; a
    partial match of 63 bases of a 64-base primer; the tie pairs of list 2;
    reads with no primer."""
    rng = random.Random(188)
    lists = directed_primers()
    recs = []

    def add(direction, seq, qual=None):
        recs.append(record(len(recs), direction, seq, qual, tile=1101 + len(recs) % 3))

    for direction, picks in ((1, WINNERS), (2, (4,))):
        for k in picks:
            p = lists[direction - 1][k]
            m = len(p)
            body = _bases(rng, 300)
            add(direction, body[:80] + p)
            add(direction, body[:80] + p + _bases(rng, 6))
            add(direction, body[:80] + p[:m // 2] + 'N' + p[m // 2 + 1:] + 'TT')
            add(direction, body[:80] + p[:m // 2] + p[m // 2 + 1:] + 'TT')
            add(direction, body[:80] + p[:m // 2] + 'A' + p[m // 2:] + 'TT')
            add(direction, body[:80] + p[:m // 2] + p[m // 2].lower() + p[m // 2 + 1:])
            for cut in (MIN_OVERLAP - 1, MIN_OVERLAP, m - 1):
                if 0 < cut < m:
                    add(direction, body[:80] + p[:cut])
            # the primer's last base in column 64, its middle on the block boundaries
            add(direction, body[:40] + p + _bases(rng, 64 - m))
            add(direction, body[:40] + p + _bases(rng, 64 - m // 2))
            add(direction, body[:40] + p + _bases(rng, 128 - m // 2))
            for n in TEXT_LENGTHS:
                add(direction, (body + p)[len(body) + m - n:])
            add(direction, body[:80] + p + 'GG', qual='F' * 5)
            add(direction, body[:80] + p + 'GG', qual='F' * (80 + m + 9))
        for n in TEXT_LENGTHS:
            add(direction, _bases(rng, n, 'ACGTN'))
    long_primer = lists[0][5]
    add(1, _bases(rng, 30) + long_primer[:63])
    add(1, long_primer[:63])
    a, c, a2, c2, _ = lists[1]
    add(2, _bases(rng, 50) + 'G' + a)                                  # full, cost 0, over partial, cost 1
    add(2, _bases(rng, 50) + a2[:10] + c2[9] + a2[11:])                # partial, cost 0, over full, cost 1
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def directed_expected():
    """(bytes, stats, base_count, score_sum, classes) by the oracles."""
    lists = directed_primers()
    censored, n, total = og_censor.censor_bytes(directed_fastq(), set())
    classes = {}
    out, stats = primer3_oracle.trim_bytes(censored, None, lists[0], lists[1], E, MIN_OVERLAP, classes=classes)
    return out, stats, n, total, classes


# ---- 3' matches at the 5' primer's lead --------------------------------------
Q22 = P5[-1] + 'CATTGGACCTGAATCGTTAGC'       # 22 bases that begin with P5's last base
Q9 = P5[-1] + 'CATTGGAC'                     # 9 bases (E[9] = 0) that begin with it
LEAD_PRIMERS3 = [P, Q22, Q9]


def lead_fastq():
    """5' primer P5 (lead 22) and then: a 3' primer that starts exactly at
    the lead (found: an empty record); Q22 / Q9 starting one base before the
    lead (its first base is the 5' primer's last: Q22 is found with its first
    base missing, cost 1, Q9 is not found); a 3' partial right behind the
    lead; the 5' primer alone (no text is left)."""
    reads = [P5 + P, P5 + P + 'GATT', P5[:-1] + Q22, P5[:-1] + Q9, P5[:-1] + Q9 + 'ACCA', P5 + P[:13], P5,
             P5 + INSERT + P, P5 + INSERT]
    return ''.join(record(i, 1 + i % 2, r) for i, r in enumerate(reads)).encode()


def lead_expected():
    """(bytes, 5' stats, 3' stats, leads, cuts) by the oracles."""
    data, _, _ = og_censor.censor_bytes(lead_fastq(), set())
    leads = primer3_oracle.leads_of(data, [P5], [P5], primer_cases.E)
    _, stats5 = primer_oracle.trim_bytes(data, [P5], [P5], primer_cases.E)
    out, stats3 = primer3_oracle.trim_bytes(data, leads, LEAD_PRIMERS3, LEAD_PRIMERS3, E, MIN_OVERLAP)
    cuts = [len(a) - len(b) - lead for a, b, lead in zip(data.split(b'\n')[1::4], out.split(b'\n')[1::4], leads)]
    return out, stats5, stats3, leads, cuts


# ---- the fuzz file -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuzz_primers():
    """(3' list 1, 3' list 2): 96 primers per list, 18 to 30 bases each."""
    rng = random.Random(331)
    return tuple([_bases(rng, rng.randint(18, 30)) for _ in range(96)] for _ in (1, 2))


@functools.lru_cache(maxsize=None)
def fuzz_fastq():
    """About 4000 records of 60 to 160 bases of both directions that end in:
    a primer of the record's list and 0 to 8 more bases; the primer with 1 to
    E[m] edits and 0 to 8 more bases; the primer's first 12 to m - 1 bases,
    one in three of them with an edit; or nothing."""
    rng = random.Random(2026)
    lists = fuzz_primers()
    recs = []
    for i in range(4000):
        direction = 1 + i % 2
        p = rng.choice(lists[direction - 1])
        m = len(p)
        kind = rng.random()
        if kind < 0.25:
            tail = p + _bases(rng, rng.randint(0, 8))
        elif kind < 0.52:
            tail = _edited(rng, p, rng.randint(1, E[m])) + _bases(rng, rng.randint(0, 8))
        elif kind < 0.78:
            tail = p[:rng.randint(MIN_OVERLAP, m - 1)]
            if rng.random() < 0.33:
                tail = _edited(rng, tail, 1)
        else:
            tail = ''
        total = rng.randint(60, 160)
        recs.append(record(i, direction, _bases(rng, total - len(tail)) + tail, tile=1101 + i % 4))
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def fuzz_expected(bad_cycles=False):
    """(trimmed bytes, stats, base_count, score_sum, records per class) of
    the fuzz file by the oracles: censor (with trim_cases.FUZZ_BAD when
    bad_cycles), then 3' primers."""
    censored, n, total = og_censor.censor_bytes(fuzz_fastq(), trim_cases.FUZZ_BAD if bad_cycles else set())
    classes = {}
    lists = fuzz_primers()
    out, stats = primer3_oracle.trim_bytes(censored, None, lists[0], lists[1], E, MIN_OVERLAP, classes=classes)
    return out, stats, n, total, classes


# ---- bad cycles, adapters, 5' and 3' primers in one call --------------------
ADAPTER = trim_cases.NEXTERA
CHAIN_PRIMERS = (['GTCAGGATCCTTACGAGCTAAC', 'TTGACCGTAAGCTAGGCTAATCGG'],
                 ['CAGTTCGGATACCGTTAAGCCT', 'AGGCTTCAGACTTGGCAATC'])


@functools.lru_cache(maxsize=None)
def chain_fastq():
    """About 300 pairs of an amplicon library with short inserts: read 1 is
    a primer of list 1, an insert of 0 to 90 bases, the reverse complement of
    a primer of list 2 and the adapter; read 2 the same from the other end.
    Reads are cut to 60 to 150 bases, so some end in the 3' primer, some in
    the adapter and some in the insert."""
    rng = random.Random(909)
    recs = []
    for i in range(300):
        f, v = rng.choice(CHAIN_PRIMERS[0]), rng.choice(CHAIN_PRIMERS[1])
        insert = _bases(rng, rng.randint(0, 90))
        template = f + insert + reverse_complement(v)
        for direction, strand in ((1, template), (2, reverse_complement(template))):
            read = (strand + ADAPTER + _bases(rng, 150))[:rng.randint(60, 150)]
            recs.append(record(i, direction, read, tile=1101 + i % 4))
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def chain_expected():
    """(bytes, adapter stats, 5' stats, 3' stats, base_count, score_sum) by
    the oracles in the order of the passes: censor, adapters, 5' primers (the
    leads), 3' primers with 'mates' lists."""
    censored, n, total = og_censor.censor_bytes(chain_fastq(), trim_cases.FUZZ_BAD)
    cut, astats = trim_oracle.trim_bytes(censored, [ADAPTER], [ADAPTER], trim_cases.MIN_OVERLAP, trim_cases.E)
    leads = primer3_oracle.leads_of(cut, CHAIN_PRIMERS[0], CHAIN_PRIMERS[1], primer_cases.E)
    _, stats5 = primer_oracle.trim_bytes(cut, CHAIN_PRIMERS[0], CHAIN_PRIMERS[1], primer_cases.E)
    mates1 = [reverse_complement(p) for p in CHAIN_PRIMERS[1]]
    mates2 = [reverse_complement(p) for p in CHAIN_PRIMERS[0]]
    out, stats3 = primer3_oracle.trim_bytes(cut, leads, mates1, mates2, E, MIN_OVERLAP)
    return out, astats, stats5, stats3, n, total

"""Inputs shared by tests/test_primer_oracle.py, tests/test_gpu_primers.py and
tests/test_gpu_shard_primers.py: the literal cases the rules were checked on,
the fuzz FASTQ and the directed records for anchored 5' primer trimming, each
with what tests/primer_oracle.py makes of it after oracle/og_censor.py (and
tests/trim_oracle.py, where adapters are set), computed once per process."""
import functools
import random

import og_censor
import primer_oracle
import trim_cases
import trim_oracle
from trim_cases import _bases, record

E = primer_oracle.error_table(0.1)
P = 'GTCAGGATCCTTACGAGCTAAC'                          # 22 bases, E[22] = 2
INSERT = _bases(random.Random(101), 70)

# (name, read, lead or None, cost): the values the rules were checked on, the
# primer list being [P] at rate 0.1
LITERALS = [
    ('exact', P + INSERT, 22, 0),
    ('one base N', P[:9] + 'N' + P[10:] + INSERT, 22, 1),
    ('one base deleted', P[:9] + P[10:] + INSERT, 21, 1),
    ('one base inserted', P[:9] + 'A' + P[9:] + INSERT, 23, 1),
    ('two substitutions', P[:4] + 'T' + P[5:15] + 'C' + P[16:] + INSERT, 22, 2),
    ('three substitutions', P[:4] + 'T' + P[5:10] + 'A' + P[11:15] + 'C' + P[16:] + INSERT, None, None),
    ('one stray base', 'T' + P + INSERT, 23, 1),
    ('two stray bases', 'TT' + P + INSERT, 24, 2),
    ('three stray bases', 'TTT' + P + INSERT, None, None),
    ('primer alone', P, 22, 0),
    ('primer cut to 20', P[:20], 20, 2),
    ('primer cut to 19', P[:19], None, None),
    ('lower case', P.lower() + INSERT, None, None),
    ('empty', '', None, None),
]


def literals_fastq():
    return ''.join(record(i, 1 + i % 2, read) for i, (_, read, _, _) in enumerate(LITERALS)).encode()


def _edited(rng, p, edits):
    """p after `edits` edits that each change it: a base replaced by another
    one, a base inserted, a base deleted."""
    p = list(p)
    for _ in range(edits):
        op, at = rng.randint(0, 2), rng.randrange(len(p))
        if op == 0:
            p[at] = rng.choice([b for b in 'ACGT' if b != p[at]])
        elif op == 1:
            p.insert(at, rng.choice('ACGT'))
        else:
            del p[at]
    return ''.join(p)


def _with_inserts(p, count):
    """p with `count` bases inserted at even distances, each different from
    the bases beside it."""
    out = list(p)
    for q in range(count, 0, -1):
        at = q * len(p) // (count + 1)
        out.insert(at, next(b for b in 'ACGT' if b not in (p[at - 1], p[at])))
    return ''.join(out)


@functools.lru_cache(maxsize=None)
def fuzz_primers():
    """(primers1, primers2): 96 primers per list, 18 to 30 bases each."""
    rng = random.Random(31)
    return tuple([_bases(rng, rng.randint(18, 30)) for _ in range(96)] for _ in (1, 2))


@functools.lru_cache(maxsize=None)
def fuzz_fastq():
    """About 4000 records of both directions: a primer of the record's list
    exact, with 1 to E[m] edits, or with E[m] + 1 to E[m] + 3 edits, or no
    primer, then an insert of 0 to 200 bases."""
    rng = random.Random(2025)
    lists = fuzz_primers()
    recs = []
    for i in range(4000):
        direction = 1 + i % 2
        p = rng.choice(lists[direction - 1])
        e = E[len(p)]
        kind = rng.random()
        if kind < 0.28:
            head = p
        elif kind < 0.62:
            head = _edited(rng, p, rng.randint(1, e))
        elif kind < 0.78:
            head = _edited(rng, p, rng.randint(e + 1, e + 3))
        else:
            head = ''
        recs.append(record(i, direction, head + _bases(rng, rng.randint(0, 200)), tile=1101 + i % 4))
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def fuzz_expected(bad_cycles=False):
    """(trimmed bytes, stats, base_count, score_sum, records per class) of
    the fuzz file by the oracles: censor (with trim_cases.FUZZ_BAD when
    bad_cycles), then primers."""
    censored, n, total = og_censor.censor_bytes(fuzz_fastq(), trim_cases.FUZZ_BAD if bad_cycles else set())
    classes = {}
    lists = fuzz_primers()
    out, stats = primer_oracle.trim_bytes(censored, lists[0], lists[1], E, classes=classes)
    return out, stats, n, total, classes


def stats_of(result):
    """trim()'s returned primer rows in the oracle's form: {(direction,
    primer index): [reads, bases]} without the primers that won nothing."""
    out, seen = {}, {}
    for row in result['primers']:
        k = seen.get(row['direction'], 0)
        seen[row['direction']] = k + 1
        if row['reads'] or row['bases']:
            out[(row['direction'], k)] = [row['reads'], row['bases']]
    return out


READ_LENGTHS = (0, 7, 8, 69, 70, 71)
WINNERS = (0, 3, 5, 63, 64, 255)


@functools.lru_cache(maxsize=None)
def directed_primers():
    """(primers1, primers2): 256 primers of 18 to 30 bases for read 1, but
    index 0 of 8 bases, index 5 of 64, and index 200 a copy of index 3; one
    primer of 64 bases for the other records."""
    rng = random.Random(87)
    one = [_bases(rng, rng.randint(18, 30)) for _ in range(256)]
    one[0] = _bases(rng, 8)
    one[5] = _bases(rng, 64)
    one[200] = one[3]
    return one, [_bases(rng, 64)]


@functools.lru_cache(maxsize=None)
def directed_fastq():
    """For the primers 0, 3 (= 200), 5, 63, 64, 255 of list 1 (every lane
    round of the kernel) and the one of list 2: the primer before an insert,
    with one edit of each kind, with E[m] inserted bases (the 64-base primers
    end at column 70), with E[m] + 1 of them, behind a stray base, cut to
    READ_LENGTHS and to m - E[m] - 1 and m - E[m] bases, with a quality line
    shorter than the lead and one longer than the sequence; and reads with no
    primer."""
    rng = random.Random(88)
    lists = directed_primers()
    recs = []

    def add(direction, seq, qual=None):
        recs.append(record(len(recs), direction, seq, qual, tile=1101 + len(recs) % 3))

    for direction, picks in ((1, WINNERS), (2, (0,))):
        for k in picks:
            p = lists[direction - 1][k]
            m, e = len(p), E[len(p)]
            tail = _bases(rng, 80)
            add(direction, p + tail)
            add(direction, p[:m // 2] + 'N' + p[m // 2 + 1:] + tail)
            add(direction, p[:m // 2] + p[m // 2 + 1:] + tail)
            add(direction, p[:m // 2] + 'A' + p[m // 2:] + tail)
            spread = _with_inserts(p, e)
            add(direction, spread + tail)
            add(direction, spread[:3] + 'G' + spread[3:] + tail)
            add(direction, 'C' + p + tail)
            for n in READ_LENGTHS + (m - e - 1, m - e):
                add(direction, (p + tail)[:n])
                add(direction, (spread + tail)[:n])
            add(direction, p + tail, qual='F' * 5)
            add(direction, p + tail[:10], qual='F' * (m + 19))
        for n in READ_LENGTHS:
            add(direction, _bases(rng, n, 'ACGTN'))
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def directed_expected():
    lists = directed_primers()
    censored, n, total = og_censor.censor_bytes(directed_fastq(), set())
    out, stats = primer_oracle.trim_bytes(censored, lists[0], lists[1], E)
    return out, stats, n, total


ADAPTER = trim_cases.NEXTERA


def both_ends_fastq():
    """Adapters and primers in one call: the adapter cut leaves fewer bases
    than the primer needs; a read trimmed at both ends; the two trims meet
    and leave an empty record; the adapter alone; the primer alone."""
    reads = [P[:10] + ADAPTER + 'GATTACAG', P + INSERT[:40] + ADAPTER + 'GATTACAG', P + ADAPTER + 'GATTACAG',
             INSERT + ADAPTER, P + INSERT]
    return ''.join(record(i, 1 + i % 2, r) for i, r in enumerate(reads)).encode()


def both_ends_expected():
    """(bytes, adapter stats, primer stats) by the oracles, adapters first."""
    censored, _, _ = og_censor.censor_bytes(both_ends_fastq(), set())
    cut, astats = trim_oracle.trim_bytes(censored, [ADAPTER], [ADAPTER], trim_cases.MIN_OVERLAP, trim_cases.E)
    out, pstats = primer_oracle.trim_bytes(cut, [P], [P], E)
    return out, astats, pstats

"""Inputs shared by tests/test_gpu_trim.py and tests/test_gpu_shard_trim.py:
the fuzz FASTQ and the directed records for 3' adapter trimming, each with
what tests/trim_oracle.py makes of it after oracle/og_censor.py (computed
once per process)."""
import functools
import random

import og_censor
import trim_oracle

NEXTERA = 'CTGTCTCTTATACACATCT'                       # 19
TRUSEQ2 = 'AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT'        # 33
MIN_OVERLAP = 3
E = trim_oracle.error_table(0.1)


def _bases(rng, n, alphabet='ACGT'):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def record(i, direction, seq, qual=None, tile=1101):
    if qual is None:
        qual = ''.join('#+5?AFG'[(i + k) % 7] for k in range(len(seq)))
    return '@M1:2:F:1:{}:{}:{} {}:N:0:1\n{}\n+\n{}\n'.format(tile, i, i, direction, seq, qual)


def _edited(rng, a, edits):
    a = list(a)
    for _ in range(edits):
        op, p = rng.randint(0, 2), rng.randrange(len(a))
        if op == 0:
            a[p] = rng.choice('ACGT')
        elif op == 1:
            a.insert(p, rng.choice('ACGT'))
        else:
            del a[p]
    return ''.join(a)


FUZZ_ADAPTERS = ([NEXTERA], [TRUSEQ2])
FUZZ_BAD = {(str(1101 + t), c) for t in range(3) for c in (-7, -6, 3, 40, 41, 42, 118, 250, 251)} | \
           {('1101', c) for c in range(200, 420)} | {('1102', -c) for c in range(150, 420)}


@functools.lru_cache(maxsize=None)
def fuzz_fastq():
    """About 4000 records: an insert of 0 to 400 bases, then the adapter of
    the record's direction in full with 0 to 3 random edits, or a prefix of
    it, or nothing, then a random tail (none after most prefixes, so they sit
    at the read's end)."""
    rng = random.Random(2024)
    recs = []
    for i in range(4000):
        direction = 1 + i % 2
        a = FUZZ_ADAPTERS[direction - 1][0]
        seq = _bases(rng, rng.randint(0, 400))
        kind = rng.random()
        if kind < 0.36:
            seq += _edited(rng, a, rng.choice([0, 0, 1, 1, 2, 3])) + _bases(rng, rng.randint(0, 30))
        elif kind < 0.70:
            seq += a[:rng.randint(MIN_OVERLAP, len(a) - 1)]
            if rng.random() < 0.1:
                seq += _bases(rng, rng.randint(1, 4))
        else:
            seq += _bases(rng, rng.randint(0, 30))
        recs.append(record(i, direction, seq, tile=1101 + i % 4))
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def fuzz_expected(bad_cycles=False):
    """(trimmed bytes, stats, base_count, score_sum, records per class) of
    the fuzz file by the oracles: censor (with FUZZ_BAD when bad_cycles), then
    trim."""
    censored, n, total = og_censor.censor_bytes(fuzz_fastq(), FUZZ_BAD if bad_cycles else set())
    classes = {}
    out, stats = trim_oracle.trim_bytes(censored, FUZZ_ADAPTERS[0], FUZZ_ADAPTERS[1], MIN_OVERLAP, E,
                                        classes=classes)
    return out, stats, n, total, classes


def fuzz_bad_rows():
    return [dict(tile=t, cycle=str(c)) for t, c in sorted(FUZZ_BAD)]


def stats_of(result):
    """trim()'s returned rows in the oracle's form: {(direction, adapter
    index): [reads, bases]} without the adapters that won nothing."""
    out, seen = {}, {}
    for row in result['adapters']:
        k = seen.get(row['direction'], 0)
        seen[row['direction']] = k + 1
        if row['reads'] or row['bases']:
            out[(row['direction'], k)] = [row['reads'], row['bases']]
    return out


READ_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 251, 300, 700)
ADAPTER_LENGTHS = (3, 19, 33, 64)


@functools.lru_cache(maxsize=None)
def directed_adapters(count):
    """(adapters1, adapters2): `count` adapters per list, of the lengths 3,
    19, 33, 64 in turn, different for the two directions; the first of list
    1 is 19 bases, the first of list 2 is 33."""
    rng = random.Random(77)
    lens1 = [19, 33, 64, 3, 19, 33, 64, 3][:count]
    lens2 = [33, 64, 3, 19, 64, 33, 19, 3][:count]
    return ([_bases(rng, m) for m in lens1], [_bases(rng, m) for m in lens2])


@functools.lru_cache(maxsize=None)
def directed_fastq(count):
    """Records of every READ_LENGTHS length for both directions, built around
    each adapter of directed_adapters(count): the adapter (cut to the read if
    need be) at offset 0, ending exactly at the read's end, a prefix of
    MIN_OVERLAP and of MIN_OVERLAP - 1 bases at the end, an N inside the
    occurrence, one edit of each kind, quality lines shorter and longer than
    the sequence, and a read with no adapter."""
    rng = random.Random(78)
    lists = directed_adapters(count)
    recs = []

    def add(direction, seq, qual=None):
        recs.append(record(len(recs), direction, seq, qual, tile=1101 + len(recs) % 3))

    for n in READ_LENGTHS:
        for direction in (1, 2):
            add(direction, _bases(rng, n, 'ACGTN'))
            for a in lists[direction - 1]:
                m = len(a)
                # at offset 0: keeps 0 (a whole adapter, or its prefix filling the read)
                add(direction, (a + _bases(rng, max(n - m, 0)))[:n])
                # ending exactly at the read's end
                add(direction, (_bases(rng, max(n - m, 0)) + a)[-n:] if n else '')
                for ov in (MIN_OVERLAP, MIN_OVERLAP - 1):
                    if n >= ov:
                        add(direction, _bases(rng, n - ov) + a[:ov])
                if n >= m + 4 and m >= 19:
                    body = _bases(rng, n - m - 4)
                    hit = a[:m // 2] + 'N' + a[m // 2 + 1:]
                    add(direction, body + hit + _bases(rng, 4))
                    add(direction, (body + a[:7] + a[8:] + _bases(rng, 5)))          # a deleted base
                    add(direction, (body + a[:7] + 'T' + a[7:] + _bases(rng, 3)))    # an inserted base
                    # quality shorter than the cut, and longer than the sequence
                    add(direction, body + a + _bases(rng, 4), qual='F' * (len(body) // 2))
                    add(direction, body + a + _bases(rng, 4), qual='F' * (n + 9))
    return ''.join(recs).encode()


@functools.lru_cache(maxsize=None)
def directed_expected(count):
    lists = directed_adapters(count)
    censored, n, total = og_censor.censor_bytes(directed_fastq(count), set())
    out, stats = trim_oracle.trim_bytes(censored, lists[0], lists[1], MIN_OVERLAP, E)
    return out, stats, n, total

"""Directed inputs for every data-dependent path of k_pileup and the k_tok_*
token aggregation (csrc/mh_pileup.hip), shared by
tests/test_oracle_pileup_paths.py (CPU: the oracle pinned to the reference's
counters of tests/golden/pileup_paths.json), tests/test_gpu_pileup_paths.py
(the kernels against both) and tests/golden/gen_pileup_paths.py (the fixture).
No GPU is needed here: the library's constants come from
mh_test_pileup_info without a context.

Every generator is seeded (random.Random), names the path it targets, and
asserts on its own rows that the path is reached: a precondition that fails
is an AssertionError, never a skip.  Sizes follow the library's constants
(K), so a changed constant moves the cases with it (and the fixture's
SHA-256 guard then asks for a regenerated fixture).

Qualities come from both sides of both cutoffs the tests use (0 and 20): the
cutoff characters themselves ('!' and '5'), cutoff - 1 (' ' and '4'),
cutoff + 1 ('"' and '6'), the gap sentinels '!' and ' ' that apply_cigar
writes, and pairs 4 and 5 apart ('1'/'5', '0'/'5', '5'/'9', '5'/':') for
merge_pairs' min_q_delta of 5.

The issue's `tokens` case asks for 12 000 pairs, one token each, every third
event the same key, and more than TOK_LDS_KEYS (8 192) distinct keys: 12 000
such pairs have 8 001 distinct keys, so that text is asserted to pass 4 096
keys and 64 KiB of token bytes (the second host copies) and the 24 000-pair
text (16 001 keys) is the one that passes TOK_LDS_KEYS.
"""
import hashlib
import json
import random
import re

import numpy as np

import oracle
from micall_amd import _native

K = _native.pileup_info()
XCH = K['xch_span']              # longest span expanded with all loads in flight
MAXOPS = K['max_ops']
INSBUF = K['ins_buf']
TOK_SLOTS = K['tok_lds_slots']
TOK_KEYS = K['tok_lds_keys']
SLACK = K['pileup_slack']
# Two launch limits the library does not report as constants; the GPU tests
# check them against the launches mh_test_pileup_info reports (wpb never
# above MAX_WPB, tokens_big on exactly TOK_BLOCKS blocks)
MAX_WPB = 16                     # k_pileup blocks hold at most 16 waves (1024 threads)
TOK_BLOCKS = 256                 # k_tok_insert / k_tok_count launch at most 256 blocks
Q_CUTOFFS = (0, 20)

QUALS = ' !"45601:9FI#'
HIGH = 'FI9:'
HEAD = '@HD\tVN:1.0\tSO:unsorted\n'


# ---- rows of a SAM text, as rows_load takes them ---------------------------
def rows_of(sam):
    """(ref_names, pairs, rows_load arguments) of a SAM text; pairs as
    oracle.matchmaker yields them (one unit each)."""
    ref_names, pairs = oracle.matchmaker(sam.splitlines(True))
    rows, units = [], []
    for r1, r2 in pairs:
        for r in (r1, r2):
            if r is None:
                units.append(-1)
            else:
                units.append(len(rows))
                rows.append(r)
    flag = [int(r[1]) for r in rows]
    ref = [ref_names.index(r[2]) for r in rows]
    pos = [int(r[3]) for r in rows]
    cig, cig_off, n_cig = [], [], []
    for r, f in zip(rows, flag):
        ops = oracle.parse_cigar(r[5]) if not (f & 4) else []
        cig_off.append(len(cig))
        n_cig.append(len(ops))
        cig += ops
    seq = ''.join(r[9] for r in rows).encode()
    qual = ''.join(r[10][:len(r[9])].ljust(len(r[9]), 'J') for r in rows).encode()
    lens = [len(r[9]) for r in rows]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if rows else []
    args = (flag, ref, pos, cig_off, n_cig, cig or [0], np.frombuffer(seq, np.uint8),
            np.frombuffer(qual, np.uint8), offs, lens, units)
    return ref_names, pairs, args


def span_cap_lens(ref_names, pairs):
    """ref_lens that hold every row: position + read length + deletions."""
    ends = [8]
    for p in pairs:
        for r in p:
            if r:
                dels = sum(int(n) for n, op in re.findall(r'(\d+)([MIDNS])', r[5]) if op == 'D')
                ends.append(int(r[3]) + len(r[9]) + dels)
    return [max(ends)] * len(ref_names)


def row_stats(args):
    """Per row: ops, reference span, [(op index, key, length)] of its I ops
    (key = read offset + pos - 1, as apply_cigar keys an insertion)."""
    flag, ref, pos, cig_off, n_cig, cig = args[:6]
    out = []
    for i in range(len(flag)):
        span = left = 0
        ins = []
        for k in range(n_cig[i]):
            w = cig[cig_off[i] + k]
            n, t = w >> 4, w & 15
            if t == 1:
                ins.append((k, left + pos[i] - 1, n))
            if t in (0, 2):
                span += n
            if t in (0, 1, 4):
                left += n
        out.append(dict(ops=n_cig[i], span=span, ins=ins, mapped=not (flag[i] & 4)))
    return out


def unit_stats(args):
    """Per unit: the row_stats of its rows (None for a missing mate)."""
    st = row_stats(args)
    units = args[10]
    return [(st[units[2 * u]] if units[2 * u] >= 0 else None,
             st[units[2 * u + 1]] if units[2 * u + 1] >= 0 else None)
            for u in range(len(units) // 2)]


def _aligned(r):
    """{reference position: (base, quality)} of a record's M ops."""
    out, left, at = {}, 0, int(r[3])
    for n, t in re.findall(r'(\d+)([MIDS])', r[5]):
        n = int(n)
        if t == 'M':
            for x in range(n):
                out[at + x] = (r[9][left + x], r[10][left + x])
        if t in 'MD':
            at += n
        if t in 'MIS':
            left += n
    return out


def quality_deltas(pairs):
    """|q1 - q2| of every overlap position where the mates' bases differ."""
    deltas = set()
    for r1, r2 in pairs:
        if r1 is None or r2 is None or (int(r1[1]) | int(r2[1])) & 4 or r1[2] != r2[2]:
            continue
        a, b = _aligned(r1), _aligned(r2)
        for p in a.keys() & b.keys():
            if a[p][0] != b[p][0]:
                deltas.add(abs(ord(a[p][1]) - ord(b[p][1])))
    return deltas


def assert_qualities(sam, pairs):
    """What every text case promises about its qualities."""
    used = set()
    for p in pairs:
        for r in p:
            if r:
                used |= set(r[10])
    for q in Q_CUTOFFS:
        assert {chr(q + 32), chr(q + 33), chr(q + 34)} <= used, (q, sorted(used))
    assert {4, 5} <= quality_deltas(pairs), sorted(quality_deltas(pairs))


# ---- record builders -------------------------------------------------------
class Builder:
    def __init__(self, seed, refs):
        """refs: [(name, length)] in @SQ order."""
        self.rng = random.Random(seed)
        self.refs = refs
        self.lines = [HEAD] + ['@SQ\tSN:{}\tLN:{}\n'.format(n, ln) for n, ln in refs]
        longest = max(ln for _, ln in refs)
        self.genome = {n: ''.join(self.rng.choices('ACGT', k=longest + SLACK + 64)) for n, _ in refs}
        self.n = 0

    def bases(self, n):
        return ''.join(self.rng.choices('ACGTN', weights=(24, 24, 24, 24, 4), k=n))

    def quals(self, n, high=False):
        return ''.join(self.rng.choices(HIGH if high else QUALS, k=n))

    def mate(self, ref, pos, ops, mut=0.08, high=None, ins_high=0.6):
        """(cigar, seq, qual) of a read at pos with ops [(n, 'M'|'I'|'D'|'S')]:
        M bases copy the reference's genome with a few changes (so mates
        mostly agree and sometimes differ), the rest are random."""
        g, at = self.genome[ref], pos - 1
        seq, qual = [], []
        for n, t in ops:
            if t == 'D':
                at += n
                continue
            if t == 'M':
                assert at + n <= len(g), (ref, pos, ops[:4])
                seg = ''.join(c if self.rng.random() >= mut else self.rng.choice('ACGTN')
                              for c in g[at:at + n])
                at += n
                hq = high if high is not None else self.rng.random() < 0.3
            else:
                seg = self.bases(n)
                hq = high if high is not None else self.rng.random() < ins_high
            seq.append(seg)
            qual.append(self.quals(n, hq))
        return ''.join('{}{}'.format(n, t) for n, t in ops), ''.join(seq), ''.join(qual)

    def rec(self, qname, flag, ref, pos, m):
        self.lines.append('\t'.join([qname, str(flag), ref, str(pos), '44', m[0], '=', '1', '0',
                                     m[1], m[2]]) + '\n')

    def unit(self, ref, pos1, ops1, pos2=None, ops2=None, flags=(99, 147), ref2=None, **kw):
        """One read pair (or a single read when ops2 is None)."""
        q = 'u{}'.format(self.n)
        self.n += 1
        self.rec(q, flags[0], ref, pos1, self.mate(ref, pos1, ops1, **kw))
        if ops2 is not None:
            self.rec(q, flags[1], ref2 or ref, pos2, self.mate(ref2 or ref, pos2, ops2, **kw))

    def raw_unit(self, ref, recs):
        """recs: [(flag, pos, (cigar, seq, qual))] under one qname."""
        q = 'u{}'.format(self.n)
        self.n += 1
        for flag, pos, m in recs:
            self.rec(q, flag, ref, pos, m)

    def disagreeing_units(self, ref, pos):
        """Mates that differ at every position with qualities 4 and 5 apart,
        at, below and above both cutoffs, and the gap sentinels as read
        qualities."""
        a, b = 'ACGTACGTACGTACGTACGTACGT', 'CATGCATGCATGCATGCATGCATG'
        for q1, q2 in (('5' * 24, '1' * 12 + '0' * 12), ('5' * 24, '9' * 12 + ':' * 12),
                       (' !"456' * 4, '456 !"' * 4), ('!' * 24, ' ' * 12 + '"' * 12),
                       ('%' * 12 + '&' * 12, '!' * 24), ('4' * 24, '0' * 24)):
            self.raw_unit(ref, [(99, pos, ('24M', a, q1)), (147, pos, ('24M', b, q2))])
            self.raw_unit(ref, [(99, pos, ('24M', a, q1)), (147, pos + 5, ('24M', a, q2))])

    def text(self):
        return ''.join(self.lines)


def ops_exact(rng, n, kinds='ID', m_len=(1, 3), x_len=(1, 3)):
    """A CIGAR of exactly n ops: M x M ... M, behind a soft clip when n is
    even; x drawn from kinds."""
    if n == 1:
        return [(30, 'M')]
    ops = [(rng.randint(1, 4), 'S')] if n % 2 == 0 else []
    k = n - len(ops)
    for j in range(k):
        if j % 2 == 0:
            ops.append((rng.randint(*m_len), 'M'))
        else:
            ops.append((rng.randint(*x_len), rng.choice(kinds)))
    assert len(ops) == n
    return ops


def ops_span(ops):
    return sum(n for n, t in ops if t in 'MD')


class Case:
    def __init__(self, name, path, sam, ref_lens=None, in_fixture=True):
        self.name, self.path, self.sam, self.in_fixture = name, path, sam, in_fixture
        self.ref_names, self.pairs, self.args = rows_of(sam)
        self.ref_lens = ref_lens or span_cap_lens(self.ref_names, self.pairs)

    def sha(self):
        data = self.sam.encode()
        return dict(sha256=hashlib.sha256(data).hexdigest(), bytes=len(data))


# ---- the cases ---------------------------------------------------------------
def case_ops():
    """More than 64 ops: the per-offset LDS walk of the expansion, ops >= 64
    read from global memory in merge_inserts, MH_MAXOPS itself."""
    b = Builder(101, [('r1', 400)])
    rng = b.rng
    sizes = (1, 2, MAXOPS // 2 - 1, MAXOPS // 2, MAXOPS // 2 + 1, MAXOPS - 1, MAXOPS)
    for n in sizes:
        for other in (n, 5, sizes[-1]):
            b.unit('r1', rng.randint(1, 40), ops_exact(rng, n), rng.randint(1, 40), ops_exact(rng, other))
        b.unit('r1', rng.randint(1, 40), ops_exact(rng, n))
    # an insertion at one key in both mates, mate 1's at op index >= 64:
    # mate 1 is (1M 1D) x 33 (read offset 33 after 66 ops), then the I
    for l1, l2 in ((3, 6), (3, 3), (6, 3), (2, 3), (3, 2)):
        lead = [(1, 'M'), (1, 'D')] * (MAXOPS // 4 + 1)
        left1 = len(lead) // 2
        ops1 = lead + [(l1, 'I'), (10, 'M')]
        ops2 = [(left1 - 20, 'M'), (l2, 'I'), (10, 'M')]
        b.unit('r1', 1, ops1, 21, ops2, high=True, mut=0.0)
    # the one-reference-op shortcut beside multi-op mates
    for short in ([(5, 'S'), (20, 'M'), (4, 'S')], [(3, 'I'), (20, 'M')], [(20, 'M'), (2, 'I')]):
        for n in (5, MAXOPS // 2 + 1):
            b.unit('r1', rng.randint(1, 30), short, rng.randint(1, 30), ops_exact(rng, n))
            b.unit('r1', rng.randint(1, 30), ops_exact(rng, n), rng.randint(1, 30), short)
        b.unit('r1', 7, short, 9, short)
    # leading deletions
    b.unit('r1', 5, [(2, 'D'), (20, 'M')], 3, [(3, 'D'), (10, 'M'), (2, 'I'), (12, 'M')])
    b.unit('r1', 5, [(2, 'D'), (20, 'M')])
    b.disagreeing_units('r1', 11)
    c = Case('ops', case_ops.__doc__, b.text())
    st = unit_stats(c.args)
    have = {r['ops'] for u in st for r in u if r}
    assert set(sizes) <= have, sorted(have)
    assert max(have) == MAXOPS
    idx = [k for u in st for r in u if r for k, _, _ in r['ins']]
    assert min(idx) < 64 <= max(idx)
    both = [u for u in st if u[0] and u[1] and
            {key for k, key, _ in u[0]['ins'] if k >= 64} & {key for _, key, _ in u[1]['ins']}]
    assert len(both) >= 5
    assert_qualities(c.sam, c.pairs)
    return c


def case_spans():
    """Reference spans around PU_XCH * 64: the serial expansion instead of the
    all-loads-in-flight one, also for one short and one long mate."""
    b = Builder(102, [('r1', 1500)])
    rng = b.rng

    def with_dels(span, read=60):
        d = span - read
        d1 = rng.randint(1, d - 1)
        return [(20, 'M'), (d1, 'D'), (20, 'M'), (d - d1, 'D'), (20, 'M')]

    for s1, s2 in ((XCH - 1, XCH - 1), (XCH, XCH), (XCH + 1, XCH + 1), (XCH + 1, XCH), (XCH, XCH + 1),
                   (XCH - 1, XCH + 1)):
        b.unit('r1', rng.randint(1, 50), with_dels(s1), rng.randint(1, 50), with_dels(s2))
        b.unit('r1', rng.randint(1, 50), [(s1, 'M')], rng.randint(1, 50), with_dels(s2))
    for s in (XCH - 1, XCH, XCH + 1):
        b.unit('r1', rng.randint(1, 50), with_dels(s), rng.randint(1, 300), [(30, 'M')])
        b.unit('r1', rng.randint(1, 300), [(30, 'M')], rng.randint(1, 50), with_dels(s))
        b.unit('r1', rng.randint(1, 50), with_dels(s))
    long1 = [(500, 'M'), (3, 'I'), (300, 'M'), (4, 'D'), (221, 'M')]
    assert sum(n for n, t in long1 if t in 'MI') == 1024
    b.unit('r1', 3, long1, 400, [(30, 'M')])
    b.unit('r1', 400, [(30, 'M')], 3, long1)
    b.unit('r1', 900, [(30, 'M')], 3, [(1024, 'M')])
    b.unit('r1', 3, long1, 200, [(700, 'M')])
    b.unit('r1', 100, [(1024, 'M')], 3, long1)
    b.unit('r1', 40, [(1024, 'M')])
    b.disagreeing_units('r1', 11)
    c = Case('spans', case_spans.__doc__, b.text())
    st = unit_stats(c.args)
    spans = {r['span'] for u in st for r in u if r}
    assert {XCH - 1, XCH, XCH + 1} <= spans
    assert any(u[0] and u[1] and u[0]['span'] > XCH and u[1]['span'] <= 60 for u in st)
    assert any(u[0] and u[1] and u[1]['span'] > XCH and u[0]['span'] <= 60 for u in st)
    assert any(u[0] and u[1] and u[0]['span'] > XCH and u[1]['span'] > XCH for u in st)
    lens = c.args[9]
    assert max(lens) == 1024 and any(r['span'] > ln for r, ln in zip(row_stats(c.args), lens))
    assert_qualities(c.sam, c.pairs)
    return c


LONG_INS = (1, 2, 3, 63, 64, 65, 66, 255, 256, 257, 258, 300, 600, 900, 1020)


def case_inserts():
    """Many and long insertions per unit: more than 4 merged insertions (the
    key loop past the four register keys), more than 64 (the loops over the
    per-wave scratch), same-key merges of every length order and quality
    outcome, and insertions as long as a 1024-base read can carry."""
    b = Builder(103, [('r1', 300)])
    rng = b.rng
    per_mate = (MAXOPS - 1) // 2       # I ops of an M I M ... M read

    def with_ins(k):
        """M I M ... M with k insertions at even read offsets: every I and
        the M behind it are 1 + 1, 3 + 1 or 2 + 2 bases, so the keys of two
        such mates at positions of different parity are distinct."""
        if not k:
            return [(30, 'M')]
        ops = [(2, 'M')]
        for _ in range(k):
            n = rng.randint(1, 3)
            ops += [(n, 'I'), (1 if n % 2 else 2, 'M')]
        return ops

    def keys(pos, ops):
        out, left = set(), 0
        for n, t in ops:
            if t == 'I':
                out.add(left + pos - 1)
            if t in 'MIS':
                left += n
        return out

    def distinct_pair(k1, k2):
        """Mates with k1 and k2 insertions, no key in common."""
        ops1, p1 = with_ins(k1), 2 * rng.randint(1, 10)
        ops2, p2 = with_ins(k2), 2 * rng.randint(1, 10) + 1
        assert not keys(p1, ops1) & keys(p2, ops2)
        return p1, ops1, p2, ops2

    for total in (0, 1, 4, 5, per_mate, per_mate + 1, per_mate + 2, 2 * per_mate):
        k1 = min(total, per_mate)
        for rep in range(2):
            p1, o1, p2, o2 = distinct_pair(k1, total - k1)
            b.unit('r1', p1, o1, p2, o2, ins_high=0.8)
            b.unit('r1', p2, o2, p1, o1, high=True)
    # three-base insertions only, so most leave a token
    p1, o1, p2, o2 = distinct_pair(per_mate, per_mate)
    o1 = [(3, 'I') if t == 'I' else (n, t) for n, t in o1]
    b.unit('r1', p1, o1, p1 + 1, [(40, 'M')], high=True, mut=0.0)
    b.unit('r1', p1, o1, high=True, mut=0.0)
    # same key in both mates: every length order, both quality outcomes
    for l1, l2 in ((3, 6), (6, 6), (6, 3), (2, 3), (3, 1), (4, 6), (1, 1), (66, 63), (63, 66)):
        for hq1, hq2 in ((True, True), (False, True), (True, False)):
            q = 'u{}'.format(b.n)
            b.n += 1
            for flag, ln, hq in ((99, l1, hq1), (147, l2, hq2)):
                c, s, ql = b.mate('r1', 30, [(8, 'M'), (ln, 'I'), (8, 'M')], high=True, mut=0.0)
                if not hq:   # one base of the insertion at / below both cutoffs
                    at = 8 + rng.randrange(ln)
                    ql = ql[:at] + rng.choice(' !') + ql[at + 1:]
                b.rec(q, flag, 'r1', 30, (c, s, ql))
    # long insertions: in mate 1 only, in mate 2 only, at one key in both
    for ln in LONG_INS:
        ops = [(2, 'M'), (ln, 'I'), (2, 'M')]
        for hq in (True, None):
            b.unit('r1', 50, ops, 48, [(30, 'M')], high=hq, mut=0.0, ins_high=1.0)
            b.unit('r1', 48, [(30, 'M')], 50, ops, high=hq, mut=0.0, ins_high=1.0)
        b.unit('r1', 50, ops, 50, ops, high=True, mut=0.0)
        b.unit('r1', 50, ops, 50, ops)
        b.unit('r1', 50, ops, high=True)
    for l1, l2 in ((258, 300), (300, 258), (900, 600), (600, 900), (1020, 3), (3, 1020), (1020, 1020),
                   (256, 258), (258, 256)):
        b.unit('r1', 50, [(2, 'M'), (l1, 'I'), (2, 'M')], 50, [(2, 'M'), (l2, 'I'), (2, 'M')],
               high=True, mut=0.0)
    b.disagreeing_units('r1', 11)
    c = Case('inserts', case_inserts.__doc__, b.text())
    st = unit_stats(c.args)
    n_keys = {len({key for r in u if r for _, key, _ in r['ins']}) for u in st}
    assert {0, 1, 4, 5, per_mate, per_mate + 1, per_mate + 2, 2 * per_mate} <= n_keys, sorted(n_keys)
    assert 2 * per_mate > 64 > 4
    lens = {(bool(u[0] and u[0]['ins']), bool(u[1] and u[1]['ins']), ln)
            for u in st for r in u if r for _, _, ln in r['ins']}
    for ln in LONG_INS:
        assert {(True, False, ln), (False, True, ln), (True, True, ln)} <= lens, ln
    assert max(c.args[9]) == 1024
    # worst case of the merged-insertion buffer for 1024-base reads
    assert 3 * max(c.args[9]) <= INSBUF
    assert_qualities(c.sam, c.pairs)
    return c


def case_windows_a():
    """One reference with an LDS window and reads past it: positions up to
    ref_len, up to ref_len + 64 (the window's end) and up to cap
    (ref_len + MH_PILEUP_SLACK) in the dense counters."""
    ref_len = 300
    b = Builder(104, [('r1', ref_len)])
    rng = b.rng
    cap = ref_len + SLACK
    for end in ([ref_len - 40, ref_len - 1, ref_len, ref_len + 1, ref_len + 63, ref_len + 64,
                 ref_len + 65, ref_len + 66, ref_len + 500, cap - 1, cap] +
                [rng.randint(60, cap) for _ in range(40)]):
        n1, n2 = rng.randint(20, 60), rng.randint(20, 60)
        ops2 = [(n2 - 14, 'M'), (3, 'I'), (5, 'M'), (2, 'D'), (4, 'M')]
        b.unit('r1', max(1, end - n1 - 20), [(n1, 'M')], end - n2 + 1, ops2)
        b.unit('r1', end - n1 + 1, [(n1, 'M')], high=True)
    b.disagreeing_units('r1', ref_len + 50)
    b.disagreeing_units('r1', cap - 40)
    c = Case('windows_a', case_windows_a.__doc__, b.text(), ref_lens=[ref_len])
    ends = {p + r['span'] - 1 for r, p in zip(row_stats(c.args), c.args[2])}
    assert max(ends) == cap
    assert any(e < ref_len for e in ends) and any(ref_len < e <= ref_len + 64 for e in ends)
    assert any(ref_len + 64 < e < cap for e in ends)
    assert_qualities(c.sam, c.pairs)
    return c


def _scatter(b, ref, ref_len, n, high=None):
    rng = b.rng
    for _ in range(n):
        n1, n2 = rng.randint(20, 60), rng.randint(20, 60)
        p = rng.randint(1, ref_len - 80)
        ops2 = [(n2 - 9, 'M'), (3, 'I'), (9, 'M')] if rng.random() < 0.3 else [(n2, 'M')]
        b.unit(ref, p, [(n1 - 5, 'M'), (2, 'D'), (5, 'M')], p + rng.randint(0, 15), ops2, high=high)


BIG_REF = 20000


def case_windows_b1():
    """A reference too long for any LDS window, alone: win_words == 0, every
    count goes to the dense counters, the n_cu * 8 grid."""
    b = Builder(105, [('big', BIG_REF)])
    _scatter(b, 'big', BIG_REF, 300)
    b.unit('big', BIG_REF - 30, [(31, 'M')], BIG_REF - 25, [(26, 'M')], high=True)
    b.disagreeing_units('big', BIG_REF - 100)
    c = Case('windows_b1', case_windows_b1.__doc__, b.text(), ref_lens=[BIG_REF])
    assert_qualities(c.sam, c.pairs)
    return c


def case_windows_b2():
    """That reference beside a short one: the short one gets a window, the
    long one (with more hits) none."""
    b = Builder(106, [('big', BIG_REF), ('small', 300)])
    _scatter(b, 'big', BIG_REF, 300)
    _scatter(b, 'small', 300, 120)
    b.disagreeing_units('big', 700)
    b.disagreeing_units('small', 100)
    c = Case('windows_b2', case_windows_b2.__doc__, b.text(), ref_lens=[BIG_REF, 300])
    assert_qualities(c.sam, c.pairs)
    return c


WIN_C_REFS, WIN_C_LEN = 16, 2000
WIN_C_TOP = (8, 13)                                   # the two most-hit references
WIN_C_TIED = (0, 1, 3, 4, 5, 7, 9, 11, 12, 15)        # equal hits behind them
WIN_C_HITS = {k: 44 if k == 8 else 38 if k == 13 else 20 if k in WIN_C_TIED else 0
              for k in range(WIN_C_REFS)}


def case_windows_c():
    """More hit references than LDS holds windows for: pile_geometry fills
    the most-hit first and skips (continue) the rest.  Two references (at
    high indices) have the most hits, ten tie behind them, four have none:
    the room runs out among the tied ones, where the lower index wins."""
    refs = [('w{}'.format(k), WIN_C_LEN) for k in range(WIN_C_REFS)]
    b = Builder(107, refs)
    hits = [WIN_C_HITS[k] for k in range(WIN_C_REFS)]
    order = [k for k in range(WIN_C_REFS) for _ in range(hits[k])]
    b.rng.shuffle(order)
    for k in order:
        _scatter(b, refs[k][0], WIN_C_LEN, 1)
    b.disagreeing_units('w{}'.format(WIN_C_TOP[1]), 1900)
    c = Case('windows_c', case_windows_c.__doc__, b.text(), ref_lens=[WIN_C_LEN] * WIN_C_REFS)
    rows = np.bincount(c.args[1], minlength=WIN_C_REFS)
    assert (rows == 0).sum() == 4 and len(WIN_C_TIED) == 10
    assert len({rows[k] for k in WIN_C_TIED}) == 1
    assert all(rows[t] > rows[WIN_C_TIED[0]] for t in WIN_C_TOP)
    assert_qualities(c.sam, c.pairs)
    return c


UNITS_BIG = 20000


def _units_text(n_units, seed=108):
    b = Builder(seed, [('r1', 200), ('r2', 200)])
    rng = b.rng
    if n_units > 100:
        b.disagreeing_units('r1', 20)
    while b.n < n_units:
        kind = b.n % 11
        p1, p2 = rng.randint(1, 170), rng.randint(1, 170)
        m = [(24, 'M')]
        if kind == 3:
            b.unit('r1', p1, m)                                          # a single mate
        elif kind == 5:
            b.unit('r1', p1, m, p2, m, flags=(69, 137))                  # first mate unmapped
        elif kind == 7:
            b.unit('r2', p1, m, p2, m, flags=(73, 133))                  # second mate unmapped
        elif kind == 8:
            b.unit('r1', p1, m, p2, m, ref2='r2')                        # mates on two references
        elif kind == 9:
            b.unit('r2', p1, [(10, 'M'), (3, 'I'), (11, 'M')], p1, [(10, 'M'), (3, 'I'), (11, 'M')])
        elif kind == 10:
            b.unit('r1', p1, m, p2, m, flags=(77, 141))                  # both unmapped
        else:
            b.unit('r1', p1, m, p1 + rng.randint(0, 12), [(20, 'M'), (2, 'D'), (4, 'M')])
    return b.text()


def case_units(n_units=UNITS_BIG):
    """Unit scheduling: more units than blocks * waves per block (a block's
    second grid stride) and, as prefixes of 1 .. 17 units, every count around
    the waves of one block; single mates, unmapped mates in first and second
    place, mates on two references."""
    name = 'units' if n_units == UNITS_BIG else 'units_{:02d}'.format(n_units)
    c = Case(name, case_units.__doc__, _units_text(n_units), ref_lens=[200, 200])
    units = c.args[10]
    assert len(units) // 2 == n_units
    if n_units == UNITS_BIG:
        flags = np.array(c.args[0]).reshape(-1)
        assert -1 in units and (flags & 4).any()
        assert max(c.args[9]) == 24
        assert_qualities(c.sam, c.pairs)
    return c


UNIT_PREFIXES = tuple(range(1, MAX_WPB + 2))


def _tokens_text(n_pairs, seed):
    """n_pairs pairs of identical high-quality mates 6M 9I 6M, one token
    each; every third pair the same read at the same position."""
    b = Builder(seed, [('r1', 200)])
    rng = b.rng
    fixed = b.mate('r1', 77, [(6, 'M'), (9, 'I'), (6, 'M')], high=True, mut=0.0)
    fixed = (fixed[0], fixed[1].replace('N', 'A'), fixed[2])
    for k in range(n_pairs):
        if k % 3 == 0:
            pos, m = 77, fixed
        else:
            pos = rng.randint(1, 150)
            seq = ''.join(rng.choices('ACGT', k=21))
            m = ('6M9I6M', seq, ''.join(rng.choices(HIGH, k=21)))
        q = 't{}'.format(k)
        b.rec(q, 99, 'r1', pos, m)
        b.rec(q, 147, 'r1', pos, m)
    return b.text()


def case_tokens(n_pairs):
    """Token aggregation: more distinct (ref, pos, token) keys than
    k_tok_count's LDS histogram holds (TOK_LDS_KEYS), more than the first
    host copy brings (4096 keys, 64 KiB of token bytes), one key joined from
    every block."""
    c = Case('tokens_{}'.format(n_pairs), case_tokens.__doc__, _tokens_text(n_pairs, 109 + n_pairs),
             ref_lens=[200])
    keys = {(r1[3], r1[9][5:15]) for r1, _ in c.pairs}
    assert len(c.pairs) == n_pairs and len(keys) > 4096
    assert 10 * len(keys) > (64 << 10)
    assert sum(1 for r1, _ in c.pairs if r1[3] == '77' and r1[9] == c.pairs[0][0][9]) >= n_pairs // 3
    return c


TOKENS_PAIRS = (12000, 24000)
# the 24 000-pair text is the one past k_tok_count's LDS histogram
assert TOKENS_PAIRS[1] * 2 // 3 > TOK_KEYS


def text_cases():
    """Every case with a SAM text, fixture order."""
    yield case_ops()
    yield case_spans()
    yield case_inserts()
    yield case_windows_a()
    yield case_windows_b1()
    yield case_windows_b2()
    yield case_windows_c()
    for n in UNIT_PREFIXES:
        yield case_units(n)
    yield case_units()
    for n in TOKENS_PAIRS:
        yield case_tokens(n)


_CACHE = {}


def cases():
    """text_cases(), built once per process and left unchanged."""
    if 'cases' not in _CACHE:
        _CACHE['cases'] = list(text_cases())
    return _CACHE['cases']


# ---- inputs that must be refused -----------------------------------------------
def error_cases():
    """(name, SAM text, ref_lens, stage, message pattern): rows_load or the
    pileup must refuse the text with that error."""
    b = Builder(110, [('r1', 400)])
    b.unit('r1', 5, ops_exact(b.rng, MAXOPS - 1), 9, [(30, 'M')])
    b.unit('r1', 5, ops_exact(b.rng, MAXOPS + 1), 9, [(30, 'M')])
    yield 'ops_{}'.format(MAXOPS + 1), b.text(), [400], 'rows_load', 'bad cigar in row 2'
    # a read one position past cap, on the first of two references (a write
    # there would land in the second one's counters)
    b = Builder(111, [('r1', 300), ('r2', 300)])
    b.unit('r1', 10, [(30, 'M')], 20, [(30, 'M')], high=True)
    b.unit('r1', 300 + SLACK - 28, [(30, 'M')], 300 + SLACK - 40, [(30, 'M')], high=True)
    yield 'past_cap', b.text(), [300, 300], 'pileup', 'malformed alignment row'
    # PU_INSBUF holds whatever two loadable reads can carry (3 x 1024): a
    # read of 1025 bases is refused when the rows are loaded
    b = Builder(112, [('r1', 300)])
    assert INSBUF >= 3 * 1024
    b.unit('r1', 10, [(4, 'M'), (1017, 'I'), (4, 'M')], 10, [(30, 'M')], high=True)
    yield 'read_1025', b.text(), [300], 'rows_load', r'length 1025 \(max 1024\)'


# ---- counters in one canonical form -----------------------------------------------
def canonical_counters(refmap):
    """JSON text of {reference: {position: {token: count}}} without empty
    positions, keys sorted; refmap values may be (pos_nucs, max_pos) (the
    oracle's) or pos_nucs (the reference's)."""
    out = {}
    for name, v in refmap.items():
        pos_nucs = v[0] if isinstance(v, tuple) else v
        out[name] = {str(p): dict(c) for p, c in pos_nucs.items() if c}
    return json.dumps(out, sort_keys=True, separators=(',', ':'))


TEXT_LIMIT = 2048


def stored(text):
    """The text itself when short, else its length and SHA-256."""
    if len(text) <= TEXT_LIMIT:
        return text
    data = text.encode()
    return dict(sha256=hashlib.sha256(data).hexdigest(), bytes=len(data))


def assert_equals_stored(text, want, what):
    if isinstance(want, str):
        assert text == want, what
        return
    data = text.encode()
    assert len(data) == want['bytes'], what
    assert hashlib.sha256(data).hexdigest() == want['sha256'], what


# ---- tokens_big: arrays, no SAM text ---------------------------------------------
TOKENS_BIG_PAIRS = TOK_BLOCKS * (TOK_SLOTS + TOK_SLOTS // 8)
TOKENS_BIG_POS = 100


def tokens_big(n_pairs=TOKENS_BIG_PAIRS):
    """The LDS table of k_tok_insert full (li < 0): more events per block
    than TOK_LDS_SLOTS, nearly all of them distinct keys.  Pairs of identical
    high-quality mates 1M 6I 1M at positions 1 .. 100 (shorter than the
    issue's 10M 3I 10M: 2.4 million rows of 23 bases took the test past a few
    seconds; the event count is unchanged and six inserted bases give the
    distinct keys three cannot: 4^7 x 100 > 1.1 million).  Pair u encodes u
    in its bases, except every 16th, which repeats the pair 5 before it.
    Returns (rows_load arguments, ref_lens, expected) with expected =
    (pos, token as 7 base codes, count) of numpy.unique over the keys."""
    u = np.arange(n_pairs, dtype=np.int64)
    src = np.where((u % 16 == 15), u - 5, u)
    pos = (src % TOKENS_BIG_POS + 1).astype(np.int32)
    digits = src // TOKENS_BIG_POS
    assert digits.max() < 4 ** 7
    codes = np.stack([(digits >> (2 * k)) & 3 for k in range(7)], axis=1).astype(np.uint8)
    lut = np.frombuffer(b'ACGT', np.uint8)
    reads = np.concatenate([lut[codes], np.full((n_pairs, 1), ord('G'), np.uint8)], axis=1)   # 8 bases
    seq = np.repeat(reads, 2, axis=0).reshape(-1)
    n_rows = 2 * n_pairs
    qual = np.full(seq.shape, ord('I'), np.uint8)
    flag = np.tile(np.array([99, 147], np.int32), n_pairs)
    cig = [(1 << 4) | 0, (6 << 4) | 1, (1 << 4) | 0]
    args = (flag, np.zeros(n_rows, np.int32), np.repeat(pos, 2), np.zeros(n_rows, np.int32),
            np.full(n_rows, 3, np.int32), cig, seq, qual, np.arange(n_rows, dtype=np.int64) * 8,
            np.full(n_rows, 8, np.int32), np.arange(n_rows, dtype=np.int64))
    # the token of a pair: its first base (position pos) + the six inserted
    key = pos.astype(np.int64)
    for k in range(7):
        key = key * 4 + codes[:, k]
    uniq, count = np.unique(key, return_counts=True)
    assert n_pairs < 100000 or (n_pairs // TOK_BLOCKS > TOK_SLOTS and
                                len(uniq) // TOK_BLOCKS > TOK_SLOTS)
    return args, [200], (uniq, count)


def tokens_big_keys(ev_raw):
    """The (key, count) arrays of a fetched pileup's ev_raw, in
    tokens_big's key encoding (every token 7 bases)."""
    ne = len(ev_raw['pos'])
    assert (ev_raw['len'] == 7).all() and (ev_raw['ref'] == 0).all()
    pool = np.frombuffer(ev_raw['pool'], np.uint8)
    tok = pool[(ev_raw['off'][:, None] + np.arange(7)[None, :]).reshape(-1)].reshape(ne, 7)
    code = np.full(256, 255, np.uint8)
    code[list(b'ACGT')] = [0, 1, 2, 3]
    codes = code[tok]
    assert (codes < 4).all()
    key = ev_raw['pos'].astype(np.int64)
    for k in range(7):
        key = key * 4 + codes[:, k]
    order = np.argsort(key)
    return key[order], ev_raw['count'][order]


def tokens_big_pairs(args):
    """SAM-style pairs of tokens_big's rows (for the oracle, small n only)."""
    flag, _, pos = args[0], args[1], args[2]
    seq = args[6].reshape(-1, 8)
    pairs = []
    for u in range(len(flag) // 2):
        rows = []
        for h in (0, 1):
            i = 2 * u + h
            rows.append(['p{}'.format(u), str(flag[i]), 'r1', str(pos[i]), '44', '1M6I1M', '=', '1', '0',
                         seq[i].tobytes().decode(), 'I' * 8])
        pairs.append(tuple(rows))
    return ['r1'], pairs

"""Directed remap.csv texts for every data-dependent path of k_s2a_merge and
the grouping kernels behind it (k_s2a_count, k_s2a_verify, k_s2a_compact,
k_s2a_gather; csrc/mh_sam2aln.hip), shared by tests/test_oracle_s2a_merge.py
(CPU: the oracle pinned to the reference's outputs of
tests/golden/s2a_merge_paths.json), tests/test_gpu_s2a_merge.py (the kernels
against the same outputs) and tests/golden/gen_s2a_merge.py (the fixture).
No GPU is needed here: the library's constants come from mh_test_sam2aln_info
without a context.

Every generator is seeded (random.Random), names the path it targets, and
asserts on its own parsed rows that the path is reached: a precondition that
fails is an AssertionError, never a skip.  Sizes follow the library's
constants (K), so a changed constant moves the cases with it (and the
fixture's SHA-256 guard then asks for a regenerated fixture).

Qualities are high ('I', 'F') wherever quality is not the point, so that
every unit reaches aligned.csv: a unit that fails the prop_N test writes no
body and tests nothing.  Only the `status*` and `unpaired` cases name units
that fail (Case.failing).

Matchmaker yields a row without a mate after every pair, so a text's single
rows are the last merge units whatever their place in the text.  Where a
single unit has to stand between pairs (the `reuse` cases), it is two rows of
one qname whose flags lack bit 1: they pair up, and the second is ignored
(sam2aln.py:362, the device's upaired).
"""
import collections
import csv
import hashlib
import io
import json
import os
import random

import og_sam2aln
from micall_amd import _native

K = _native.sam2aln_info()
LDS = K['lds_bytes']
BLOCK_CAP = K['block_cap']
WPB = K['wpb_max']
MIN_TABLE = K['min_table']
MAX_CUTS = K['max_cuts']
SPAN_B = K['span_bytes']
OP_B = K['op_bytes']

HEAD = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'
EDGES = (1, 63, 64, 65, 127, 128, 129)      # either side of one and two 64-lane chunks
OTHER = {'A': 'C', 'C': 'G', 'G': 'T', 'T': 'A'}


def wave_bytes(span, ops):
    """LDS bytes of one wave for a longest reference span and op count, as
    s2a_run sizes them (asserted against the launch by the GPU tests)."""
    cap = (max(span, 1) + 15) & ~15
    return (SPAN_B * cap + OP_B * (max(ops, 1) + 1) + 15) & ~15


def wpb_of(wb):
    """Waves per block for wave_bytes wb; 0: refused."""
    if wb > LDS:
        return 0
    w = WPB
    while w > 1 and w * wb > LDS:
        w -= 1
    return w


def cigar_of(ops):
    return ''.join('{}{}'.format(n, t) for n, t in ops)


def ops_exact(rng, n, lens=(1, 3)):
    """A CIGAR of exactly n >= 5 ops: a leading and a trailing S around
    M x M ... M with x drawn from D and I (an M split in two when n is odd)."""
    body = n - 2
    ops = [(rng.randint(1, 3), 'S')]
    if body % 2 == 0:
        ops.append((rng.randint(*lens), 'M'))
        body -= 1
    for j in range(body):
        ops.append((rng.randint(*lens), 'M' if j % 2 == 0 else rng.choice('DI')))
    ops.append((rng.randint(1, 3), 'S'))
    assert len(ops) == n and ops[-2][1] == 'M'
    return ops


class Text:
    """A remap.csv text as a list of units (each a list of rows)."""

    def __init__(self, seed, refs=('R',), genome=600):
        self.rng = random.Random(seed)
        self.genome = {r: ''.join(self.rng.choices('ACGT', k=genome)) for r in refs}
        self.units = []
        self.n = 0

    def read(self, ref, pos, ops, q='I'):
        """(cigar, seq, qual) of a read at pos: M bases copy the reference's
        genome (mates agree wherever they overlap), I and S bases are random."""
        g, at = self.genome[ref], max(pos - 1, 0)
        seq = []
        for n, t in ops:
            if t == 'D':
                at += n
            elif t == 'M':
                assert at + n <= len(g), (ref, pos, at, n)
                seq.append(g[at:at + n])
                at += n
            else:
                seq.append(''.join(self.rng.choices('ACGT', k=n)))
        seq = ''.join(seq)
        return cigar_of(ops), seq, ''.join(self.rng.choice(q) for _ in seq)

    def name(self, name=None):
        self.n += 1
        return name or 'u{}'.format(self.n - 1)

    def raw(self, recs, name=None):
        """recs: [(flag, rname, pos, (cigar, seq, qual))] under one qname."""
        qn = self.name(name)
        self.units.append([[qn, str(flag), ref, str(pos), '44', m[0], '=', '1', '0', m[1], m[2]]
                           for flag, ref, pos, m in recs])
        return qn

    def pair(self, ref, pos1, ops1, pos2, ops2, q='I', name=None, flags=(99, 147)):
        return self.raw([(flags[0], ref, pos1, self.read(ref, pos1, ops1, q)),
                         (flags[1], ref, pos2, self.read(ref, pos2, ops2, q))], name)

    def single(self, ref, pos, ops, q='I', name=None, flag=0):
        return self.raw([(flag, ref, pos, self.read(ref, pos, ops, q))], name)

    def single_between(self, ref, pos, ops, q='I', name=None):
        """A single unit that keeps its place among the pairs: two unpaired
        rows of one qname, the second (another shape altogether) ignored."""
        other = self.read(ref, pos + 3, [(5, 'S'), (40, 'M'), (3, 'D'), (9, 'M')], q)
        return self.raw([(0, ref, pos, self.read(ref, pos, ops, q)), (16, ref, pos + 3, other)], name)

    def text(self, reverse=False):
        out = io.StringIO()
        w = csv.writer(out, lineterminator='\n')
        for u in (reversed(self.units) if reverse else self.units):
            w.writerows(u)
        return HEAD + out.getvalue()


# ---- what a text's units look like to the merge ------------------------------
def units_of(text):
    """[(row1, row2 or None)] in matchmaker order."""
    return list(og_sam2aln.matchmaker(csv.DictReader(io.StringIO(text))))


def _padded(row):
    pos = int(row['pos']) - 1
    s, _, _ = og_sam2aln.apply_cigar(row['cigar'], row['seq'], row['qual'])
    return '-' * pos + s


def shape(unit):
    """Of a unit the host hands to the merge: single, the op counts and
    reference spans of its rows, and for a pair merge_pairs' view of it: len1
    <= len2 (after the role swap), the two pads, swapped, fwd_start and
    rev_start (None: never)."""
    r1, r2 = unit
    paired = int(r1['flag']) & 1
    rows = (r1, r2) if paired else (r1,)
    ops = [len(og_sam2aln._TOKEN.findall(r['cigar'])) for r in rows]
    pads = [max(int(r['pos']) - 1, 0) for r in rows]
    seqs = [_padded(r) for r in rows]
    out = dict(single=not paired, ops=ops, span=[len(s) - p for s, p in zip(seqs, pads)], pads=pads,
               lens=[len(s) for s in seqs])
    if paired:
        s1, s2 = seqs
        out['swapped'] = len(s1) > len(s2)
        if out['swapped']:
            s1, s2 = s2, s1
        out['len1'], out['len2'] = len(s1), len(s2)
        out['rev_start'] = next((i for i, c in enumerate(s2) if c != '-'), None)
        out['fwd_start'] = next((i for i in range(len(s1)) if not (s1[i] == '-' and s2[i] == '-')), None)
    return out


def merged_units(text):
    """The units that reach the device (no host-decided failure cause)."""
    out = []
    for r1, r2 in units_of(text):
        paired = int(r1['flag']) & 1
        if paired and r2 is None:
            continue
        if r1['cigar'] == '*' or (r2 is not None and r2['cigar'] == '*'):
            continue
        if paired and r1['rname'] != r2['rname']:
            continue
        out.append((r1, r2))
    return out


class Case:
    """name, the path it targets, the text, the q-cutoff lists to run it at;
    failing: the qnames failed.csv may (and must) hold; raises: the reference
    raises on it (the all-gap unit); refused: the library's own refusal
    (no reference value), a pattern of its message."""

    def __init__(self, name, path, text, lists, failing=(), raises=False, refused=None):
        self.name, self.path, self.text, self.lists = name, ' '.join(path.split()), text, [list(c) for c in lists]
        self.failing, self.raises, self.refused = frozenset(failing), raises, refused
        self.units = merged_units(text)
        self.shapes = [shape(u) for u in self.units]

    def sha(self):
        data = self.text.encode()
        return dict(sha256=hashlib.sha256(data).hexdigest(), bytes=len(data))


# ---- reuse: one wave, many units of different shape ------------------------------
REUSE_UNITS = 40
REUSE_MAX_BLOCKS = (1, 2)       # mh_test_set_sam2aln's cap: 10 and 5 units per wave


def _reuse_builder():
    b = Text(201, genome=900)
    rng = b.rng
    k = 0
    while len(b.units) < REUSE_UNITS:
        kind, p = k % 8, rng.randint(1, 30)
        k += 1
        if kind == 0:      # a long pair with a deletion and an insertion
            b.pair('R', p, [(120, 'M'), (7, 'D'), (100, 'M'), (3, 'I'), (20, 'M')],
                   p + rng.randint(0, 90), [(230, 'M')])
        elif kind == 1:    # one base
            b.pair('R', p, [(1, 'M')], p, [(1, 'M')])
        elif kind == 2:    # a single unit between pairs (mt[1] of the unit before must not stand)
            b.single_between('R', p, [(30, 'M')])
        elif kind == 3:    # 130 ops: the third round of the lane scan
            b.pair('R', p, ops_exact(rng, 130), p + rng.randint(0, 9), ops_exact(rng, 130))
        elif kind == 4:    # the forward read never starts
            gap = ('12M', '-' * 12, 'I' * 12)
            b.raw([(99, 'R', p, gap), (147, 'R', p + 11 + rng.randint(1, 80), b.read('R', p + 40, [(25, 'M')]))])
        elif kind == 5:    # short again
            b.pair('R', p, [(8, 'M')], p + 2, [(8, 'M')])
        elif kind == 6:    # a long first mate over a short second one: the roles swap
            b.pair('R', p, [(200, 'M')], p + 60, [(3, 'S'), (20, 'M')])
        else:              # a single long read of many ops
            b.single_between('R', p, ops_exact(rng, 65, lens=(2, 4)))
    return b


def _assert_reuse(c):
    sh = c.shapes
    assert len(sh) == REUSE_UNITS, len(sh)
    assert max(max(s['ops']) for s in sh) >= 129
    singles = [i for i, s in enumerate(sh) if s['single']]
    pairs = [i for i, s in enumerate(sh) if not s['single']]
    # single units between pairs, in the first wave's turn after a pair
    assert singles and min(singles) < max(pairs) and any(i - 1 in pairs for i in singles)
    assert any(not s['single'] and s['span'] == [1, 1] for s in sh)
    assert any(not s['single'] and s['fwd_start'] is None for s in sh)
    assert any(not s['single'] and s['swapped'] for s in sh)
    assert max(max(s['span']) for s in sh) > 200
    for blocks in REUSE_MAX_BLOCKS:
        assert len(sh) >= 5 * blocks * WPB


def case_reuse(reverse=False):
    """The unit loop's second and later turns: a wave reuses its LDS arrays
    (c0 q0 c1 q1, opref, opread) for units of another shape, a pair after a
    single unit and a single unit after a pair; run with the merge limited to
    1 and 2 blocks (mh_test_set_sam2aln), forwards and in reversed order."""
    c = Case('reuse_reversed' if reverse else 'reuse', case_reuse.__doc__,
             _reuse_builder().text(reverse), [[15], [15, 10, 0]])
    _assert_reuse(c)
    return c


SHORT = 8


def case_reuse_natural():
    """The same loop without the hook: one unit whose span leaves room for
    one wave per block, then more 8-base pairs than the block cap, so that
    some wave takes a second unit (and the loop's stride is the grid's)."""
    span = _span_for(1, low=True)
    b = Text(202, genome=span + 64)
    b.pair('R', 1, [(20, 'M'), (span - 40, 'D'), (20, 'M')], 5, [(30, 'M')])
    rng = b.rng
    n_short = BLOCK_CAP + 16
    bodies = [''.join(rng.choices('ACGT', k=SHORT)) for _ in range(300)]
    rows = []
    for k in range(n_short):
        body = bodies[min(rng.randrange(600), 299)]     # half of them one body, the rest spread
        pos = 1 + k % 3
        for flag in (99, 147):
            rows.append(['s{}'.format(k), str(flag), 'R', str(pos), '44', '8M', '=', '1', '0', body, 'IIIIFFII'])
    b.units.append(rows)
    c = Case('reuse_natural', case_reuse_natural.__doc__, b.text(), [[15]])
    wb = wave_bytes(max(max(s['span']) for s in c.shapes), 3)
    assert wpb_of(wb) == 1
    assert len(c.units) == n_short + 1 and len(c.units) > BLOCK_CAP * 1
    assert len({(u[0]['pos'], u[0]['seq']) for u in c.units}) > 500
    return c


# ---- wpb: the LDS budget's steps ----------------------------------------------
WPB_OPS = 3


def _span_for(wpb, low):
    """The shortest (low) or longest reference span whose wave_bytes (with
    WPB_OPS ops at most) gives wpb waves per block; wpb 0: refused."""
    spans = [s for s in range(16, LDS // SPAN_B + 64, 16) if wpb_of(wave_bytes(s, WPB_OPS)) == wpb]
    return (spans[0] - 15) if low else spans[-1]


def _wpb_text(seed, span):
    b = Text(seed, genome=span + 200)
    rng = b.rng
    for k in range(7):
        p = rng.randint(1, 40)
        if k == 2:
            b.pair('R', 1, [(20, 'M'), (span - 40, 'D'), (20, 'M')], 9, [(40, 'M')])
        else:
            b.pair('R', p, [(30, 'M'), (2, 'D'), (20, 'M')], p + rng.randint(0, 25), [(45, 'M')])
    return b.text()


def wpb_cases():
    """Spans either side of every step of wpb = 4, 3, 2, 1 (wpb * wave_bytes
    against the LDS budget; readfirstlane(threadIdx.x >> 6) indexes the wave's
    slice) through one D op, among ordinary overlapping pairs that fill the
    other wave slots; and one span past the last step, which is refused."""
    out = []
    for wpb in range(WPB, 0, -1):
        for low in (True, False):
            if wpb == WPB and low:
                continue          # every other case
            span = _span_for(wpb, low)
            c = Case('wpb_{}_{}'.format(wpb, 'low' if low else 'high'), wpb_cases.__doc__,
                     _wpb_text(210 + 2 * wpb + low, span), [[15]])
            c.wpb = wpb
            got = max(max(s['span']) for s in c.shapes)
            assert got == span and max(max(s['ops']) for s in c.shapes) == WPB_OPS
            assert wpb_of(wave_bytes(got, WPB_OPS)) == wpb
            # one position more (high) or less (low) is another wpb
            assert wpb_of(wave_bytes(span + (-1 if low else 1), WPB_OPS)) != wpb or (low and wpb == WPB)
            assert len(c.units) > WPB
            out.append(c)
    span = _span_for(1, low=False) + 1
    c = Case('wpb_refused', wpb_cases.__doc__, _wpb_text(219, span), [[15]],
             refused=r'reference span \d+ too long for LDS')
    c.wpb = 0
    assert wpb_of(wave_bytes(span, WPB_OPS)) == 0
    out.append(c)
    assert [x.wpb for x in out] == [4, 3, 3, 2, 2, 1, 1, 0]
    return out


# ---- ops: more than 64 ops ----------------------------------------------------
OPS_SIZES = (63, 64, 65, 127, 128, 129, 200)


def case_ops():
    """CIGARs of more than 64 ops: the second and later rounds of
    apply_cigar's lane scan with its rf0 / rd0 carry from lane 63, the search
    over many ops (ops of length 0 among them) in the expansion; rows whose
    CIGAR consumes no reference."""
    b = Text(220, genome=900)
    rng = b.rng
    for n in OPS_SIZES:
        p = rng.randint(1, 30)
        b.pair('R', p, ops_exact(rng, n), p + rng.randint(0, 9), [(60, 'M')])
        b.pair('R', p + 4, [(60, 'M')], p, ops_exact(rng, n))
        b.pair('R', p, ops_exact(rng, n), p + 2, ops_exact(rng, n))
        b.single('R', p, ops_exact(rng, n, lens=(2, 5)))
    # ops of length 0
    g = b.genome['R']
    b.raw([(99, 'R', 3, ('0S5M0D3M0I2M0M', g[2:12], 'I' * 10)), (147, 'R', 3, ('0M10M', g[2:12], 'F' * 10))])
    b.raw([(99, 'R', 3, ('0M10M', g[2:12], 'I' * 10)), (147, 'R', 5, ('0S5M0D3M0I2M0M', g[4:14], 'F' * 10))])
    zeros = [(0, 'S')] + [(1, 'M'), (0, 'D'), (0, 'I')] * 33 + [(0, 'M')]
    b.pair('R', 7, zeros, 9, [(40, 'M')])
    # no reference consumed
    b.raw([(99, 'R', 4, ('5I', 'ACGTA', 'IIIII')), (147, 'R', 6, b.read('R', 6, [(20, 'M')]))])
    b.raw([(99, 'R', 6, b.read('R', 6, [(20, 'M')])), (147, 'R', 4, ('4S', 'ACGT', 'IIII'))])
    c = Case('ops', case_ops.__doc__, b.text(), [[15], [10, 15]])
    for n in OPS_SIZES:
        assert sum(1 for s in c.shapes if not s['single'] and s['ops'][0] == n) >= 2, n
        assert sum(1 for s in c.shapes if not s['single'] and s['ops'][1] == n) >= 2, n
        assert any(s['ops'] == [n, n] for s in c.shapes)
        assert any(s['single'] and s['ops'] == [n] for s in c.shapes)
    assert max(max(s['ops']) for s in c.shapes) == 200 > 128
    assert any(0 in s['span'] for s in c.shapes)
    assert any('0D' in u[0]['cigar'] for u in c.units) and any(s['ops'][0] == len(zeros) for s in c.shapes)
    return c


# ---- edges64: the chunk edges of the three position loops --------------------------
def case_edges64():
    """Lengths, pads and gaps at 1, 63, 64, 65, 127, 128 and 129: the start
    scan's exit (rev_start and fwd_start in different 64-position chunks),
    the merge loops that begin at lo, the n fill between mates that do not
    overlap, leading '-' of a D-led alignment, pos 0 and -3."""
    b = Text(230, genome=900)
    for v in EDGES:
        b.pair('R', 1, [(v, 'M')], 1, [(v, 'M')])                     # a.len == len2 == v
        b.pair('R', 1, [(v, 'M')], 1, [(v + 1, 'M')])                 # a.len == v, len2 == v + 1
        b.pair('R', 1, [(v + 1, 'M')], 1, [(v, 'M')])                 # swapped
        b.pair('R', v + 1, [(20, 'M')], v + 6, [(20, 'M')])           # pad1 == v
        b.pair('R', 3, [(20, 'M')], v + 1, [(30, 'M')])               # pad2 == v
        b.pair('R', v + 1, [(40, 'M')], 3, [(v + 20, 'M')])           # the reverse mate starts first
        b.pair('R', 1, [(10, 'M')], 11 + v, [(10, 'M')])              # a gap of v between the mates
        b.pair('R', 5, [(10, 'M')], 15 + v, [(v, 'M')])               # and len2 - a.len around the edges
        b.pair('R', 1, [(v, 'D'), (10, 'M')], 1, [(v + 30, 'M')])     # '-' from a leading D in seq1
        b.pair('R', 1, [(v + 30, 'M')], 2, [(v, 'D'), (40, 'M')])     # and in seq2: rev_start past it
        b.pair('R', 1, [(v, 'D'), (10, 'M')], 1, [(v, 'D'), (12, 'M')])   # both: fwd_start == rev_start == v
        b.single('R', v + 1, [(v, 'M')])
        # the forward read (all '-') never starts, the reverse one v past its end
        b.raw([(99, 'R', 1, ('{}M'.format(v), '-' * v, 'I' * v)),
               (147, 'R', 2 * v + 1, b.read('R', 2 * v + 1, [(v + 1, 'M')]))])
    for pos in (0, -3):
        b.pair('R', pos, [(20, 'M')], 3, [(20, 'M')])
        b.pair('R', 3, [(20, 'M')], pos, [(70, 'M')])
        b.single('R', pos, [(66, 'M')])
    c = Case('edges64', case_edges64.__doc__, b.text(), [[15], [0, 15]])
    pairs = [s for s in c.shapes if not s['single']]
    for v in EDGES:
        assert any(s['len1'] == v and s['len2'] == v for s in pairs), v
        assert any(s['len1'] == v and s['len2'] == v + 1 and not s['swapped'] for s in pairs), v
        assert any(s['len1'] == v and s['swapped'] for s in pairs), v
        assert any(s['pads'][0] == v for s in pairs) and any(s['pads'][1] == v for s in pairs), v
        assert any(s['rev_start'] is not None and s['rev_start'] - s['len1'] == v for s in pairs), v
        assert any(s['fwd_start'] == v == s['rev_start'] for s in pairs), v
        assert any(s['fwd_start'] is None and s['rev_start'] == 2 * v for s in pairs), v
    # the two starts in different chunks, with a.len past the first chunk
    assert any(s['fwd_start'] is not None and s['fwd_start'] < 64 <= s['rev_start'] and s['len1'] > 64
               for s in pairs)
    assert any(s['fwd_start'] is None and s['rev_start'] >= 128 and s['len1'] >= 64 for s in pairs)
    assert any(int(u[0]['pos']) < 0 for u in c.units) and any(int(u[0]['pos']) == 0 for u in c.units)
    return c


# ---- roles -------------------------------------------------------------------------
def case_roles():
    """merge_pairs' roles: row 1 longer than row 2 (swapped), equal lengths,
    row 2 longer; the forward read never starting (a first mate of '-' with
    real qualities: ibase = a.len, mlen = len2 - a.len) with the reverse
    mate's first base before, at, after and 70 and more past a.len."""
    b = Text(240, genome=700)
    rng = b.rng
    for l1, l2 in ((50, 30), (40, 40), (30, 50), (130, 64), (64, 64), (64, 130), (2, 1), (1, 2)):
        for p1, p2 in ((1, 1), (5, 1), (1, 5)):
            b.pair('R', p1, [(l1, 'M')], p2, [(l2, 'M')])
            b.pair('R', p1, [(l1 - 1, 'M'), (2, 'D'), (1, 'M')], p2, [(l2, 'M')], q='IF')
    for n in (5, 64, 70):
        for p1 in (1, 4):
            alen = p1 - 1 + n
            for first in (alen - 3, alen - 1, alen, alen + 1, alen + 2, alen + 70, alen + 129):
                if first < 0:
                    continue
                b.raw([(99, 'R', p1, ('{}M'.format(n), '-' * n, ''.join(rng.choice('IF5') for _ in range(n)))),
                       (147, 'R', first + 1, b.read('R', first + 1, [(n + 10, 'M')]))])
    c = Case('roles', case_roles.__doc__, b.text(), [[15]])
    pairs = [s for s in c.shapes if not s['single']]
    assert any(s['swapped'] for s in pairs) and any(s['lens'][0] == s['lens'][1] for s in pairs)
    assert any(s['lens'][0] < s['lens'][1] for s in pairs)
    never = [s for s in pairs if s['fwd_start'] is None]
    assert {s['rev_start'] - s['len1'] for s in never} >= {0, 1, 2, 70, 129}
    late = [s for s in pairs if s['fwd_start'] is not None and s['fwd_start'] == s['rev_start'] and
            s['pads'][1] in (s['len1'] - 3, s['len1'] - 1)]
    assert len(late) >= 6
    return c


# ---- quals: the cutoff arithmetic ----------------------------------------------------
QUAL_LISTS = ([15], [0, 93], [15, 10, 0], [0, 10, 15, 20], [0, 10, 14, 15, 16], [30, 0, 15, 20, 10, 5],
              [0, 5, 10, 15, 20, 25, 30], [40, 0, 5, 10, 15, 20, 25, 30])
QUAL_T = 12


def case_quals(cuts):
    """thr > cut at its edges: qualities at each cutoff - 1, the cutoff and
    the cutoff + 1, mates that agree and that disagree with dq of -5, -4, 0, 4
    and 5 (the tie that gives N), the bytes ' ', '!' and '~', a '-' the read
    itself holds that moves the offset between cutoffs; n_cut below and at
    the bound of every k_s2a_merge<NC> instance.  A deletion both mates share
    (merged '-', counted by the stripped length) keeps every unit under
    max_prop_n even at cutoff 93, where no base survives."""
    b = Text(250 + len(cuts) + sum(cuts))
    rng = b.rng
    spots = []
    for cq in cuts:
        for q in (cq + 32, cq + 33, cq + 34):
            for d in (-5, -4, 0, 4, 5):
                if 32 <= q <= 126 and 32 <= q + d <= 126:
                    spots += [(True, q, q + d), (False, q, q + d), (False, q + d, q)]
    for qa in (32, 33, 126):
        for qb in (32, 33, 38, 73, 121, 126):
            spots += [(True, qa, qb), (False, qa, qb), (False, qb, qa)]
    rng.shuffle(spots)
    for k in range(0, len(spots), QUAL_T):
        part = spots[k:k + QUAL_T]
        n = len(part)
        s1 = ''.join(rng.choices('ACGT', k=n))
        s2 = ''.join(c if same else OTHER[c] for c, (same, _, _) in zip(s1, part))
        q1 = ''.join(chr(x) for _, x, _ in part)
        q2 = ''.join(chr(x) for _, _, x in part)
        cigar = '{}M{}D1M'.format(n, 2 * n + 2)
        pos = 1 + (k // QUAL_T) % 3
        b.raw([(99, 'R', pos, (cigar, s1 + 'G', q1 + 'I')), (147, 'R', pos, (cigar, s2 + 'G', q2 + 'I'))])
    # a gap the read holds, at a quality between the list's cutoffs
    mid = chr(max(sorted(cuts)[len(cuts) // 2] + 33, 40))
    b.raw([(99, 'R', 1, ('8M18D1M', '--GTACGTG', mid * 2 + 'IIIIIII')),
           (147, 'R', 1, ('8M18D1M', 'ACGTACGTG', '!!IIIIIII'))], name='gap')
    c = Case('quals_' + '_'.join(map(str, cuts)), case_quals.__doc__, b.text(), [cuts])
    assert 1 <= len(cuts) <= MAX_CUTS
    used = {ch for u in c.units for r in u for ch in r['qual']}
    assert {' ', '!', '~'} <= used
    for cq in cuts:
        assert {chr(x) for x in (cq + 32, cq + 33, cq + 34) if x <= 126} <= used, cq
    deltas = {ord(y) - ord(x) for u in c.units for x, y, s, t in
              zip(u[0]['qual'], u[1]['qual'], u[0]['seq'], u[1]['seq']) if s != t}
    assert {-5, -4, 0, 4, 5} <= deltas
    return c


assert sorted({len(c) for c in QUAL_LISTS}) == [1, 2, 3, 4, 5, 6, 7, 8] and MAX_CUTS == 8


# ---- status -----------------------------------------------------------------------------
STATUS_LENGTHS = (2, 10, 64, 65)


def case_status():
    """The prop_N test at its edge: exactly max_prop_n (0.5) passes, since the
    reference tests '>', one N more fails, at stripped lengths 2, 10, 64 and
    65, for pairs (N by quality) and single reads (N in the read); a unit that
    passes at cutoff 0 only, so that lo comes from another cutoff than the
    first; a unit that fails everywhere."""
    b = Text(260)
    g = b.genome['R']
    failing = []
    for n in STATUS_LENGTHS:
        for extra in (0, 1):
            bad = n // 2 + extra
            at = (n - bad) // 2
            for pos in (1, 4):
                seq = g[pos - 1:pos - 1 + n]
                qual = 'I' * at + '!' * bad + 'I' * (n - at - bad)
                name = '{}_{}_{}'.format('fail' if extra else 'pass', n, pos)
                b.raw([(99, 'R', pos, ('{}M'.format(n), seq, qual)), (147, 'R', pos, ('{}M'.format(n), seq, qual))],
                      name='p' + name)
                ns = seq[:at] + 'N' * bad + seq[at + bad:]
                b.raw([(0, 'R', pos, ('{}M'.format(n), ns, 'I' * n))], name='s' + name)
                if extra:
                    failing += ['p' + name, 's' + name]
    # Q1 ('"') beats cutoff 0 alone
    for pos in (1, 4):
        seq = g[pos - 1:pos + 19]
        qual = '"' * 12 + 'I' * 8
        failing.append(b.raw([(99, 'R', pos, ('20M', seq, qual)), (147, 'R', pos, ('20M', seq, qual))],
                             name='only0_{}'.format(pos)))
        failing.append(b.raw([(99, 'R', pos, ('20M', seq, '!' * 20)), (147, 'R', pos, ('20M', seq, '!' * 20))],
                             name='never_{}'.format(pos)))
    b.pair('R', 2, [(30, 'M')], 6, [(30, 'M')])
    c = Case('status', case_status.__doc__, b.text(), [[15], [15, 10, 0], [0, 15]], failing=failing)
    assert len(failing) == len(set(failing)) == 2 * 2 * len(STATUS_LENGTHS) + 4
    return c


def case_status_allgap():
    """A unit whose merged sequence is all gaps: ZeroDivisionError in the
    reference, 'all gaps (float division by zero)' here, between two good
    pairs."""
    b = Text(261)
    b.pair('R', 2, [(30, 'M')], 6, [(30, 'M')])
    b.raw([(99, 'R', 3, ('4M', '----', 'IIII')), (147, 'R', 3, ('4M', '----', 'IIII'))], name='allgap')
    b.pair('R', 4, [(30, 'M')], 9, [(30, 'M')])
    return Case('status_allgap', case_status_allgap.__doc__, b.text(), [[15]], raises=True)


# ---- distinct: the grouping's discrimination ----------------------------------------------
DISTINCT_LEN = 130
DISTINCT_FAMILIES = 10
DISTINCT_REPEAT = 1000
DISTINCT_LISTS = ([15], [10, 15])


def case_distinct():
    """Bodies that must stay distinct: equal except for the offset, the
    length (one a prefix of the other), one byte (first, last, at 62 .. 65),
    the order of the same characters (h1 and h2 are position-keyed sums), the
    reference, and through a quality edge the cutoff; every variant with its
    own multiplicity of 1 .. 9, so counts tie and the rank order falls to the
    offset and then the string; one body 1000 times.  With two cutoffs more
    than 256 distinct (reference, cutoff, body) groups, so an 8-bit key must
    collide."""
    b = Text(270, refs=('R', 'R2'))
    rng = b.rng
    L = DISTINCT_LEN
    variants = []

    def emit(rname, pos, seq, qual=None):
        mult = 1 + len(variants) % 9
        variants.append((rname, pos, seq, mult))
        cigar = '{}M'.format(len(seq))
        for _ in range(mult):
            b.raw([(99, rname, pos, (cigar, seq, qual or 'I' * len(seq))),
                   (147, rname, pos, (cigar, seq, qual or 'F' * len(seq)))])

    for _ in range(DISTINCT_FAMILIES):
        body = ''.join(rng.choices('ACGT', k=L))
        for pos in (1, 2, 65):
            emit('R', pos, body)
        emit('R', 1, body[:-1])
        emit('R', 1, body[:-2])
        for k in (0, 62, 63, 64, 65, L - 1):
            emit('R', 1, body[:k] + OTHER[body[k]] + body[k + 1:])
        i = 20
        j = next(x for x in range(90, L) if body[x] != body[i])
        swapped = list(body)
        swapped[i], swapped[j] = swapped[j], swapped[i]
        emit('R', 1, ''.join(swapped))
        assert body[::-1] != body
        emit('R', 1, body[::-1])
        emit('R2', 1, body)
        # Q12 at one position: N at cutoff 15, the base body itself at 10
        emit('R', 1, body, qual='I' * 70 + '-' + 'I' * (L - 71))
    for _ in range(DISTINCT_REPEAT):
        b.raw([(99, 'R', 7, ('20M', 'ACGTTGCAACGTTGCAACGT', 'I' * 20)),
               (147, 'R', 7, ('20M', 'ACGTTGCAACGTTGCAACGT', 'F' * 20))])
    rng.shuffle(b.units)
    c = Case('distinct', case_distinct.__doc__, b.text(), DISTINCT_LISTS)
    per_family = 15
    assert len(variants) == per_family * DISTINCT_FAMILIES
    assert len({v[:3] for v in variants}) == len(variants) - DISTINCT_FAMILIES    # the quality edge repeats a body
    # (reference, cutoff, body) groups at [10, 15]: every variant at 15, all but the edge's at 10
    assert 2 * len(variants) - DISTINCT_FAMILIES + 2 > 256
    # ties: one count at two offsets, and at one offset for two strings
    by_count = collections.defaultdict(list)
    for rname, pos, seq, mult in variants:
        if rname == 'R':
            by_count[mult].append(pos)
    assert sum(1 for p in by_count.values() if len(set(p)) > 1) >= 6
    assert all(len(p) > len(set(p)) for p in by_count.values())
    assert len(c.units) == sum(v[3] for v in variants) + DISTINCT_REPEAT
    return c


def case_table(n):
    """Exactly n merge entries either side of the grouping table's minimum
    (tsize doubles past MIN_TABLE / 2 entries): 8-base pairs, every fourth
    body a repeat."""
    b = Text(280 + n % 7)
    rng = b.rng
    bodies = []
    for k in range(n):
        if k % 4 == 3:
            body = bodies[rng.randrange(len(bodies))]
        else:
            body = ''.join('ACGT'[(k >> (2 * x)) & 3] for x in range(SHORT))
        bodies.append(body)
        b.raw([(99, 'R', 1 + k % 2, ('8M', body, 'I' * 8)), (147, 'R', 1 + k % 2, ('8M', body, 'F' * 8))])
    c = Case('table_{}'.format(n), case_table.__doc__, b.text(), [[15]])
    assert len(c.units) == n
    c.tsize = MIN_TABLE if 2 * n <= MIN_TABLE else 2 * MIN_TABLE
    return c


TABLE_SIZES = (MIN_TABLE // 2, MIN_TABLE // 2 + 1)


# ---- unpaired ---------------------------------------------------------------------------
def case_unpaired():
    """Rows whose flags lack bit 1 (single units, no cutoff applied: low
    qualities and N pass as they are), leftovers that never find their mate
    (unmatched), a '*' CIGAR, mates on two references, among passing pairs."""
    b = Text(290, refs=('R', 'S'))
    rng = b.rng
    failing = []
    for k in range(24):
        p = rng.randint(1, 40)
        kind = k % 8
        if kind == 0:
            b.single('R', p, [(30, 'M')], q='!#', flag=0)
        elif kind == 1:
            b.single('R', p, [(3, 'S'), (20, 'M'), (2, 'D'), (5, 'M'), (2, 'I'), (6, 'M')], q=' !~', flag=16)
        elif kind == 2:
            failing.append(b.single('R', p, [(30, 'M')], flag=99, name='unmatched{}'.format(k)))
        elif kind == 3:
            m = b.read('R', p, [(30, 'M')])
            failing.append(b.raw([(99, 'R', p, m), (147, 'R', p, ('*', m[1], m[2]))], name='star{}'.format(k)))
        elif kind == 4:
            failing.append(b.raw([(99, 'R', p, b.read('R', p, [(30, 'M')])),
                                  (147, 'S', p, b.read('S', p, [(30, 'M')]))], name='tworefs{}'.format(k)))
        elif kind == 5:
            b.single_between('S', p, [(25, 'M')], q='#5')
        elif kind == 6:
            seq = b.genome['R'][p - 1:p + 19]
            b.raw([(0, 'R', p, ('20M', seq[:5] + 'NNNNNNNNNN' + seq[15:], '!' * 20))])     # 10 / 20: passes
        else:
            b.pair('R', p, [(30, 'M')], p + 4, [(30, 'M')])
        b.pair('S', p, [(20, 'M'), (1, 'D'), (9, 'M')], p + rng.randint(0, 9), [(25, 'M')])
    m = b.read('R', 5, [(12, 'M')])
    failing.append(b.raw([(0, 'R', 5, ('*', m[1], m[2]))], name='star_single'))
    c = Case('unpaired', case_unpaired.__doc__, b.text(), [[15], [0, 10, 15]], failing=failing)
    assert sum(1 for s in c.shapes if s['single']) >= 12
    assert len(failing) == 10
    return c


# ---- the insertion table's collision report -----------------------------------------------
def ins_collision_text(n=400):
    """Pairs with one three-base insertion each, in the first mate alone, at
    many positions: more distinct (position, string) rows of conseq_ins.csv
    than an 8-bit key has values (the caller asserts that on the oracle's
    output).  No fixture: tests/ins_oracle.py is the expected value."""
    b = Text(295)
    for k in range(n):
        p = 1 + k % 40
        b.pair('R', p, [(10, 'M'), (3, 'I'), (12, 'M')], p + 2, [(24, 'M')])
    return b.text()


# ---- all of them -----------------------------------------------------------------------------
def all_cases():
    yield case_reuse()
    yield case_reuse(reverse=True)
    yield case_reuse_natural()
    yield from wpb_cases()
    yield case_ops()
    yield case_edges64()
    yield case_roles()
    for cuts in QUAL_LISTS:
        yield case_quals(cuts)
    yield case_status()
    yield case_status_allgap()
    yield case_distinct()
    for n in TABLE_SIZES:
        yield case_table(n)
    yield case_unpaired()


_CACHE = {}


def cases():
    """all_cases(), built once per process and left unchanged."""
    if 'cases' not in _CACHE:
        _CACHE['cases'] = list(all_cases())
        names = [c.name for c in _CACHE['cases']]
        assert len(set(names)) == len(names)
    return _CACHE['cases']


def by_name(name):
    return next(c for c in cases() if c.name == name)


def runs():
    """(case, q-cutoff list) of every run with outputs to compare."""
    return [(c, cuts) for c in cases() if not c.refused for cuts in c.lists]


def run_id(run):
    return '{}-{}'.format(run[0].name, '_'.join(map(str, run[1])))


# ---- the fixture ---------------------------------------------------------------------------------
TEXT_LIMIT = 2048


def stored(text):
    """The text itself when short, else its length and SHA-256 (the
    convention of tests/golden/gen_golden_qcuts.py)."""
    if len(text) <= TEXT_LIMIT:
        return text
    data = text.encode()
    return dict(sha256=hashlib.sha256(data).hexdigest(), bytes=len(data))


def fixture():
    """{case name: its entry} of tests/golden/s2a_merge_paths.json (layout:
    tests/golden/gen_s2a_merge.py)."""
    if 'fixture' not in _CACHE:
        here = os.path.dirname(os.path.abspath(__file__))
        with open(os.path.join(here, 'golden', 's2a_merge_paths.json')) as f:
            _CACHE['fixture'] = {c['name']: c for c in json.load(f)['cases']}
    return _CACHE['fixture']


def want_of(run):
    """The fixture's entry of a (case, q-cutoff list)."""
    c, cuts = run
    return next(r for r in fixture()[c.name]['runs'] if r['q_cutoffs'] == list(cuts))


def assert_equals_stored(text, want, what, oracle_text=None):
    """text equals a stored output; where only its digest is stored and the
    caller has the oracle's text (pinned to the same digest by
    tests/test_oracle_s2a_merge.py), a mismatch names the first line that
    differs from it."""
    if isinstance(want, str):
        assert text == want, what
        return
    data = text.encode()
    if len(data) == want['bytes'] and hashlib.sha256(data).hexdigest() == want['sha256']:
        return
    if oracle_text is not None:
        got, exp = text.splitlines(), oracle_text.splitlines()
        k = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
        raise AssertionError('{}: {} lines for {}, line {}: {!r} for {!r}'.format(
            what, len(got), len(exp), k, got[k][:200] if k < len(got) else None,
            exp[k][:200] if k < len(exp) else None))
    raise AssertionError('{}: {} bytes for {}'.format(what, len(data), want['bytes']))

"""Seeded SAM texts and watched positions for the debug reports of
remap.sam_to_conseqs (remap.py:169-225, 302-306), shared by
tests/golden/gen_debug_reports.py (the reference's strings, the fixture
tests/golden/debug_reports.json), tests/test_debug_reports_host.py (CPU) and
tests/test_gpu_sam_to_conseqs.py (k_pileup's watching instances).

watched() restates the watched count in Python from the reference's
documented behaviour: matchmaker's units, merge_reads' choice of mates,
each mate in reference coordinates, the merged sequence, update_counts' walk
over it and `qual1[pos-1] if pos <= len(qual1) else qual2[pos-1]`.  It gives
the [keys][4][95] counts and first units the device gives, and notes which
of the situations below each text reaches; covered() asserts that the set of
texts reaches every one.  No GPU is needed here.
"""
import hashlib
import json
import random
import re

import numpy as np

import og_sam2aln
import oracle

QBINS, Q0 = 95, 32
NEVER = np.iinfo(np.int64).max
Q_CUTOFFS = (0, 20)
N_TEXTS = 30
REFS = ('r1', 'r2', 'r3')          # r3 never receives a read
QUALS = ' !"45601:9FI#'
HEAD = '@HD\tVN:1.0\tSO:unsorted\n' + ''.join('@SQ\tSN:{}\tLN:900\n'.format(r) for r in REFS)

# every situation the set of texts must reach (the issue's list)
FACTS = ('disagree_pick', 'disagree_N', 'past_qual1', 'q_space', 'q_bang', 'ins3', 'mseq_N',
         'mseq_-', 'mseq_n', 'single', 'two_refs', 'unmapped_mate', 'lead_D', 'shift', 'off64',
         'off128', 'span320', 'two_keys_one_ref', 'keys_two_refs', 'key_no_reads')


def _span(cigar):
    return sum(int(n) for n, op in re.findall(r'(\d+)([MIDS])', cigar) if op in 'MD')


def watched(sam, q_cutoff, keys, facts=None):
    """(counts uint32 [keys][4][95], first_unit int64 [keys][4][95]) of the
    (rname, pos) keys over the SAM text; `facts` (a set) gains the names of
    the situations met at the keys."""
    counts = np.zeros((len(keys), 4, QBINS), dtype=np.uint32)
    first = np.full((len(keys), 4, QBINS), NEVER, dtype=np.int64)
    at = {}
    for k, key in enumerate(keys):
        at.setdefault(tuple(key), []).append(k)
    facts = set() if facts is None else facts
    names = [k[0] for k in at]
    for name in set(names):
        if names.count(name) > 1:
            facts.add('two_keys_one_ref')
    if len(set(names)) > 1:
        facts.add('keys_two_refs')
    _ref_names, units = oracle.matchmaker(sam.splitlines(True))
    with_reads = set()
    for u, (row1, row2) in enumerate(units):
        if row2 and row1[2] != row2[2]:
            facts.add('two_refs')
            continue
        mapped = [r for r in (row1, row2) if r and not int(r[1]) & 4]
        if not mapped:
            continue
        rname = mapped[0][2]
        with_reads.add(rname)
        padded, ins3 = [], set()
        for r in mapped:
            seq, qual, ins = og_sam2aln.apply_cigar(r[5], r[9], r[10])
            pad = int(r[3]) - 1
            padded.append(('-' * pad + seq, '!' * pad + qual))
            ins3.update(left + pad for left, (text, _q) in ins.items() if len(text) % 3 == 0)
        (seq1, qual1), (seq2, qual2) = padded[0], padded[1] if len(padded) > 1 else ('', '')
        mseq = og_sam2aln.merge_pairs(seq1, seq2, qual1, qual2, q_cutoff)
        shift = max(len(seq1), len(seq2)) - len(mseq)
        started = None
        hit = False
        for pos, nuc in enumerate(mseq, 1):
            if started is None:
                if nuc == '-':
                    continue
                started = pos
            ks = at.get((rname, pos))
            if ks is None:
                continue
            hit = True
            if shift:
                facts.add('shift')
            if nuc in 'nN-':
                facts.add('mseq_' + nuc)
                both = [s[pos - 1] for s, _q in padded if pos <= len(s)]
                if (nuc == 'N' and not shift and len(both) == 2 and both[0] != both[1]
                        and '-' not in both and 'N' not in both
                        and abs(ord(qual1[pos - 1]) - ord(qual2[pos - 1])) < 5):
                    facts.add('disagree_N')
                continue
            q = qual1[pos - 1] if pos <= len(qual1) else qual2[pos - 1]
            code = 'ACGT'.index(nuc)
            for k in ks:
                counts[k, code, ord(q) - Q0] += 1
                first[k, code, ord(q) - Q0] = min(first[k, code, ord(q) - Q0], u)
            both = [s[pos - 1] for s, _q in padded if pos <= len(s)]
            if not shift and len(both) == 2 and both[0] != both[1] and '-' not in both and 'N' not in both:
                facts.add('disagree_pick')
            if pos > len(qual1):
                facts.add('past_qual1')
            if q in ' !':
                facts.add('q_space' if q == ' ' else 'q_bang')
            if pos in ins3:
                facts.add('ins3')
            if pos - started >= 64:
                facts.add('off64')
            if pos - started >= 128:
                facts.add('off128')
        if hit:
            if row2 is None:
                facts.add('single')
            elif len(mapped) == 1:
                facts.add('unmapped_mate')
            if any(re.match(r'\d+D', r[5]) for r in mapped):
                facts.add('lead_D')
            if any(_span(r[5]) > 320 for r in mapped):
                facts.add('span320')
    if any(name not in with_reads for name in names):
        facts.add('key_no_reads')
    return counts, first


class Text:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.lines = [HEAD]
        self.keys = []
        self.n = 0
        self.genome = {r: ''.join(self.rng.choice('ACGT') for _ in range(900)) for r in REFS}

    def bases(self, ref, pos, cigar, err=0.0):
        """SEQ following the reference under the CIGAR's M ops."""
        out, at = [], pos - 1
        for n, op in re.findall(r'(\d+)([MIDS])', cigar):
            n = int(n)
            if op == 'M':
                for x in range(n):
                    b = self.genome[ref][at + x]
                    out.append(self.rng.choice('ACGT') if self.rng.random() < err else b)
                at += n
            elif op == 'D':
                at += n
            else:
                out.append(''.join(self.rng.choice('ACGT') for _ in range(n)))
        return ''.join(out)

    def row(self, qname, flag, ref, pos, cigar, seq=None, qual=None, err=0.0):
        seq = self.bases(ref, pos, cigar, err) if seq is None else seq
        qual = 'F' * len(seq) if qual is None else qual
        self.lines.append('\t'.join([qname, str(flag), ref, str(pos), '44', cigar, '=', '1', '0',
                                     seq, qual]) + '\n')

    def pair(self, ref, pos1, cig1, pos2, cig2, **kw):
        self.n += 1
        q = 'p{}'.format(self.n)
        self.row(q, 99, ref, pos1, cig1, **{k[:-1]: v for k, v in kw.items() if k.endswith('1')})
        self.row(q, 147, ref, pos2, cig2, **{k[:-1]: v for k, v in kw.items() if k.endswith('2')})

    def key(self, ref, pos):
        if (ref, pos) not in self.keys:
            self.keys.append((ref, pos))

    def text(self):
        return ''.join(self.lines)


def _swap(base):
    return 'ACGT'[('ACGT'.index(base) + 1) % 4]


def make(seed):
    """One text of at most 60 pairs and its keys: the directed units (their
    positions vary with the seed), then random overlapping pairs."""
    t = Text(seed)
    rng = t.rng
    g = t.genome
    a = rng.randrange(1, 40)
    # mates disagree at a: qualities 5 apart (the better one wins) and 4 apart ('N')
    for q1, q2, at in (('F', '5', a + 5), ('1', '5', a + 9), ('5', ':', a + 5)):
        s1 = t.bases('r1', a, '30M')
        s2 = s1[:at - a] + _swap(s1[at - a]) + s1[at - a + 1:]
        qa = 'F' * (at - a) + q1 + 'F' * (29 - (at - a))
        qb = 'F' * (at - a) + q2 + 'F' * (29 - (at - a))
        t.pair('r1', a, '30M', a, '30M', seq1=s1, qual1=qa, seq2=s2, qual2=qb)
        t.key('r1', at)
    # mate 1 reaches past mate 0's end; mate 0 starts after mate 1 ('!' before it)
    t.pair('r1', a + 10, '20M', a, '50M')
    t.key('r1', a + 2)        # q == '!': mate 0 has not started
    t.key('r1', a + 40)       # past len(qual1)
    # mate 0 has a deletion where mate 1 has a base: q == ' '
    t.pair('r1', a, '12M2D16M', a, '30M')
    t.key('r1', a + 12)
    # both deleted ('-'); both of low quality ('N'); a gap between the mates ('n')
    t.pair('r2', a, '12M2D16M', a, '12M2D16M')
    t.key('r2', a + 13)
    t.pair('r2', a + 40, '20M', a + 40, '20M', qual1='#' * 20, qual2='!' * 20)
    t.key('r2', a + 45)
    t.pair('r2', a + 70, '10M', a + 90, '10M')
    t.key('r2', a + 84)
    # a 3-nt insertion after read base 20: the token's position is a + 19
    t.pair('r2', a, '20M3I20M', a, '20M3I20M')
    t.key('r2', a + 19)
    # a single read, a pair on two references, an unmapped mate
    t.n += 1
    t.row('s{}'.format(t.n), 0, 'r1', a + 100, '40M')
    t.key('r1', a + 110)
    t.n += 1
    t.row('x{}'.format(t.n), 99, 'r1', a + 100, '40M')
    t.row('x{}'.format(t.n), 147, 'r2', a + 100, '40M')
    t.n += 1
    t.row('m{}'.format(t.n), 73, 'r1', a + 105, '30M')
    t.row('m{}'.format(t.n), 133, 'r1', a + 105, '*', seq=g['r1'][:30])
    # a CIGAR that starts with D
    t.pair('r1', a + 100, '2D30M', a + 104, '30M')
    # mate 0 is gaps only (4S3D): the forward read never starts, so the merged
    # sequence is mate 1 past mate 0's end and its positions shift by 7 + a
    t.pair('r2', a + 1, '4S3D', a + 40, '30M')
    t.key('r2', 2)
    t.key('r2', 6)
    t.key('r2', a + 5)
    # long mates: keys 64 and 128 positions past the first counted one
    t.pair('r1', a + 200, '150M', a + 200, '150M')
    t.key('r1', a + 270)
    t.key('r1', a + 335)
    # a mate spanning more than 320 reference positions
    t.pair('r2', a + 200, '60M270D60M', a + 480, '50M')
    t.key('r2', a + 250)
    t.key('r2', a + 540)
    # a reference without reads
    t.key('r3', a + 5)
    # random overlapping pairs with errors, indels and every quality
    for _ in range(rng.randrange(10, 38)):
        ref = rng.choice(('r1', 'r2'))
        p1 = rng.randrange(1, 200)
        p2 = p1 + rng.randrange(0, 60)
        cigs = []
        for _m in range(2):
            left, ops = rng.randrange(40, 150), []
            while left > 0:
                m = min(left, rng.randrange(10, 60))
                ops.append('{}M'.format(m))
                left -= m
                if left > 5 and rng.random() < 0.4:
                    n = rng.choice((1, 2, 3, 3, 6))
                    ops.append('{}{}'.format(n, rng.choice('ID')))
            cigs.append(''.join(ops))
        seqs = [t.bases(ref, p, c, err=0.1) for p, c in zip((p1, p2), cigs)]
        quals = [''.join(rng.choice(QUALS) for _ in s) for s in seqs]
        t.pair(ref, p1, cigs[0], p2, cigs[1], seq1=seqs[0], qual1=quals[0], seq2=seqs[1], qual2=quals[1])
    for _ in range(rng.randrange(4, 10)):
        t.key(rng.choice(('r1', 'r2')), rng.randrange(1, 330))
    assert t.n <= 60
    return t.text(), t.keys


_CACHE = {}


def cases():
    """[(name, sam, quality cutoff, keys)]: N_TEXTS seeded texts, cutoffs
    alternating, and the two debug_reports calls of the reference's
    remap_test.py."""
    if 'cases' not in _CACHE:
        out = []
        for seed in range(N_TEXTS):
            sam, keys = make(1000 + seed)
            out.append(('seeded{}'.format(seed), sam, Q_CUTOFFS[seed % 2], keys))
        _CACHE['cases'] = out
    return _CACHE['cases']


def sha(sam):
    return hashlib.sha256(sam.encode()).hexdigest()


def golden_cases(path):
    """The cases of tests/golden/debug_reports.json as dicts (name, sam,
    quality_cutoff, keys, reports).  The fixture stores a seeded text as its
    SHA-256 only: the text and its keys are generated again here and must be
    the ones the reference answered."""
    with open(path) as f:
        stored = json.load(f)['cases']
    mine = {name: (sam, q, keys) for name, sam, q, keys in cases()}
    out = []
    for c in stored:
        c = dict(c)
        if 'sam' not in c:
            sam, q, keys = mine[c['name']]
            assert sha(sam) == c['sam_sha256'] and q == c['quality_cutoff'], c['name']
            assert [list(k) for k in keys] == c['keys'], c['name']
            c['sam'] = sam
        out.append(c)
    return out


def covered():
    """Every situation of FACTS is reached by some text (an AssertionError
    names the missing ones); returns {fact: texts that reach it}."""
    reached = {f: 0 for f in FACTS}
    for _name, sam, q, keys in cases():
        facts = set()
        watched(sam, q, keys, facts)
        for f in facts:
            reached[f] += 1
    missing = [f for f, n in reached.items() if not n]
    assert not missing, missing
    return reached

"""Mate rescue, path by path (k_rescue): the register-blocked diagonal scan
of reads up to 256 nt, the strided scan of longer ones, the 2-bit scan of
mates and windows with ambiguous bases, and the rescue candidates that are
not extended again because the main pass already failed on the same (strand,
reference, diagonal).  Every case maps a few hundred directed pairs over a
small seeded reference and compares every field and CIGAR word of
ctx.fetch() with the CPU oracle (og_map) on the same reads.

The mate to rescue carries a substitution every 15 bases: no exact 22-mer
(no seed, no main-pass alignment), about m / 15 mismatches (above
--score-min), so only the rescue can align it.  Its anchor is an exact
100-mer.  Every case asserts that map_stats()[4] reaches the number of pairs
built for rescue, so none passes without running the path."""
import numpy as np
import pytest

import oracle
from micall_amd import _native

pytestmark = pytest.mark.gpu

COMP = str.maketrans('ACGTN', 'TGCAN')
LA = 100                      # anchor length
LENGTHS = (31, 32, 33, 63, 64, 65, 250, 251, 256, 257, 300)   # 257 and 300: the strided scan
RESIDUES = (0, 1, 15, 16, 17, 31)


def revcomp(s):
    return s.translate(COMP)[::-1]


def random_ref(rng, n):
    return ''.join(rng.choice(list('ACGT'), size=n))


def substituted(seq, every, phase, keep=()):
    """A copy with a substitution at phase, phase + every, ... (not inside
    the half-open spans of `keep`)."""
    out = list(seq)
    for i in range(phase, len(out), every):
        if out[i] in 'ACGT' and not any(a <= i < b for a, b in keep):
            out[i] = 'ACGT'[('ACGT'.index(out[i]) + 1) % 4]
    return ''.join(out)


class Pairs:
    """Interleaved pairs: an exact anchor and a mate taken from the
    reference coordinates the case names."""

    def __init__(self, ref, rng):
        self.ref, self.rng = ref, rng
        self.seqs, self.quals = [], []

    def add(self, anchor, mate, mate_first=False):
        qa, qm = 'I' * len(anchor), 'I' * len(mate)
        if mate_first:
            self.seqs += [mate, anchor]
            self.quals += [qm, qa]
        else:
            self.seqs += [anchor, mate]
            self.quals += [qa, qm]

    def forward_anchor(self, a_st, b_st, m, tweak=None):
        """Anchor forward at a_st (window [a_st, a_st + maxins)), the mate
        from [b_st, b_st + m) on the reverse strand."""
        x = substituted(self.ref[b_st:b_st + m], 15, int(self.rng.integers(0, 15)))
        assert len(x) == m
        if tweak:
            x = tweak(x)
        self.add(self.ref[a_st:a_st + LA], revcomp(x), mate_first=len(self.seqs) % 4 == 2)

    def reverse_anchor(self, a_end, b_st, m, tweak=None):
        """Anchor reverse ending at a_end (window [a_end - maxins, a_end)),
        the mate from [b_st, b_st + m) on the forward strand."""
        x = substituted(self.ref[b_st:b_st + m], 15, int(self.rng.integers(0, 15)))
        assert len(x) == m
        if tweak:
            x = tweak(x)
        self.add(revcomp(self.ref[max(0, a_end - LA):a_end]), x, mate_first=len(self.seqs) % 4 == 2)

    @property
    def n_pairs(self):
        return len(self.seqs) // 2


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def assert_same(gpu, want):
    assert gpu.shape == want.shape
    for f in _native.ALN_FIELDS:
        if not np.array_equal(gpu[f], want[f]):
            i = int(np.nonzero(gpu[f] != want[f])[0][0])
            raise AssertionError((i, f, int(gpu[f][i]), int(want[f][i])))
    used = np.arange(want['cigar'].shape[1])[None, :] < want['n_cigar'][:, None]
    bad = np.nonzero(((gpu['cigar'] != want['cigar']) & used).any(axis=1))[0]
    assert len(bad) == 0, (int(bad[0]), _native.cigar_text(gpu[bad[0]]), _native.cigar_text(want[bad[0]]))


def run(ctx, refs, seqs, quals, mode=oracle.E2E, maxins=1200, paired=True):
    """Maps on the device and on the oracle, asserts equality, returns the
    oracle's records."""
    assert len(seqs) <= 8000
    names = ['r%d' % i for i in range(len(refs))]
    ix = oracle.Index(refs, oracle.seed_len(mode))
    want = np.frombuffer(bytes(oracle.map_reads(ix, oracle.params(mode, maxins=maxins), seqs, quals, paired)),
                         dtype=_native.ALN_DTYPE)[:len(seqs)]
    ctx.index_build(names, refs, oracle.seed_len(mode))
    ctx.reads_load(seqs, quals, paired)
    ctx.map(_native.params(mode, maxins=maxins))
    assert_same(ctx.fetch(), want)
    return want


@pytest.mark.parametrize('maxins', [300, 1200, 2600])
def test_scan_shapes(ctx, maxins):
    """Every mate length around the 32-base word edges, both anchor strands,
    every window start residue, windows clipped at the reference's first and
    last base, a window of exactly m bases (one diagonal).  With -X 2600 the
    diagonals pass 1024 and the mates lie in the second and third chunk."""
    rng = np.random.default_rng(100 + maxins)
    L = 4000
    ref = random_ref(rng, L)
    P = Pairs(ref, rng)
    for m in LENGTHS:
        if m > maxins:
            continue
        for r in RESIDUES:
            for rep in range(2):
                # anchor forward, window [lo, lo + maxins)
                lo = 320 + r
                span = min(lo + maxins, L) - lo - m          # last diagonal of the window
                first = min(1100, span) if maxins == 2600 else 0
                off = span if rep == 0 and r == 0 else int(rng.integers(first, span + 1))
                P.forward_anchor(lo, lo + off, m)
                # anchor reverse, window [lo, lo + maxins)
                off = 0 if rep == 0 and r == 0 else int(rng.integers(first, span + 1))
                P.reverse_anchor(lo + maxins, lo + off, m)
    for m in (33, 250, 251, 256, 257):
        if m > maxins:
            continue
        # clipped at the first base (mates at it and inside), at the last base
        a_end = min(maxins, 700)
        P.reverse_anchor(a_end, 0, m)
        P.reverse_anchor(a_end, int(rng.integers(0, a_end - m + 1)), m)
        a_st = L - min(maxins, 600) + 7
        P.forward_anchor(a_st, L - m, m)
        P.forward_anchor(a_st, int(rng.integers(a_st, L - m + 1)), m)
        # a window of exactly m bases: one diagonal
        P.forward_anchor(L - m, L - m, m)
        P.reverse_anchor(m, 0, m)
    want = run(ctx, [ref], P.seqs, P.quals, maxins=maxins)
    assert ctx.map_stats()[4] >= P.n_pairs, (ctx.map_stats(), P.n_pairs)
    assert (want['flag'] & 4 == 0).mean() > 0.9     # the rescues align


@pytest.mark.parametrize('mode', [oracle.E2E, oracle.LOCAL])
@pytest.mark.parametrize('period', [3, 8])
def test_ties_leftmost(ctx, mode, period):
    """A window over tandem repeats: the mate matches equally well every
    `period` diagonals, inside one lane's block of 16 diagonals and across
    the blocks of many lanes; the leftmost maximum must win."""
    rng = np.random.default_rng(200 + period)
    unit = random_ref(rng, period)
    while len(set(unit)) < 2:
        unit = random_ref(rng, period)
    ref = random_ref(rng, 700) + unit * (1500 // period) + random_ref(rng, 700)
    rep0, rep1 = 700, 700 + period * (1500 // period)
    P = Pairs(ref, rng)
    for k in range(60):
        m = (250, 251, 256, 64, 33, 300)[k % 6]
        b_st = int(rng.integers(rep0 + 40, rep1 - m - 40))
        if k % 2:
            P.forward_anchor(int(rng.integers(rep0 - 400, rep0 - LA)), b_st, m)
        else:
            P.reverse_anchor(int(rng.integers(rep1 + LA, rep1 + 400)), b_st, m)
    run(ctx, [ref], P.seqs, P.quals, mode=mode, maxins=2000)
    assert ctx.map_stats()[4] >= P.n_pairs, (ctx.map_stats(), P.n_pairs)


def test_ambiguous_bases(ctx):
    """An N in the mate and an N in the window go to the 2-bit scan; an N
    that lies past the window's end leaves the bit-plane scan in charge."""
    rng = np.random.default_rng(300)
    L = 3000
    base = random_ref(rng, L)
    lo = 400
    # (a) N in the mate, (b) N inside the window, (c) the only N two bases past the window's end
    in_window = base[:lo + 600] + 'N' + base[lo + 601:]
    past_end = base[:lo + 1202] + 'N' + base[lo + 1203:]
    total = 0
    for ref, tweak in ((base, lambda x: x[:20] + 'N' + x[21:]), (in_window, None), (past_end, None)):
        P = Pairs(ref, rng)
        for m in (33, 64, 250, 251, 256, 300):
            for k in range(6):
                b_st = int(rng.integers(lo, lo + 1200 - m + 1))
                if ref is in_window and lo + 600 - m < b_st <= lo + 600:
                    b_st = lo + 601          # the mate itself stays free of N
                if ref is past_end and k == 0:
                    b_st = lo + 1200 - m     # the last diagonal, next to the N
                P.forward_anchor(lo, b_st, m, tweak)
                P.reverse_anchor(lo + 1200, b_st, m, tweak)
        run(ctx, [ref], P.seqs, P.quals)
        assert ctx.map_stats()[4] >= P.n_pairs, (ctx.map_stats(), P.n_pairs)
        assert ctx.rescue_skipped() == 0
        total += P.n_pairs
    assert total <= 4000


M_SKIP = 248     # 226 - 19 k is no multiple of the seed interval 19: see the palindrome case
SEED_AT = 95     # a seed offset of a 248-nt read (5 x 19)


def failing_mate(segment):
    """`segment` with one exact seed window at SEED_AT and a substitution
    every 7 bases elsewhere (32 > 26 mismatches at quality 'I': below
    --score-min).  The base before the window is substituted, so the
    reverse complement holds no exact 22-mer at a seed offset of its own."""
    return substituted(segment, 7, 3, keep=[(SEED_AT, SEED_AT + 22)])


def test_skip_repeated_extension(ctx):
    """Mates with one exact seed: the main pass extends the true diagonal
    and fails, the rescue finds the same diagonal and does not extend it
    again; the records equal the oracle's, which runs the extension."""
    rng = np.random.default_rng(400)
    ref = random_ref(rng, 3000)
    P = Pairs(ref, rng)
    for k in range(120):
        a_st = int(rng.integers(100, 1500))
        b_st = a_st + int(rng.integers(0, 1200 - M_SKIP + 1))
        x = failing_mate(ref[b_st:b_st + M_SKIP])
        if k % 2:
            P.add(ref[a_st:a_st + LA], revcomp(x), mate_first=k % 4 == 1)
        else:
            a_end = min(b_st + M_SKIP + int(rng.integers(0, 600)), len(ref))
            P.add(revcomp(ref[a_end - LA:a_end]), x, mate_first=k % 4 == 0)
    # among them pairs whose mate is rescued (no seed, few mismatches)
    for k in range(40):
        a_st = int(rng.integers(100, 1500))
        P.forward_anchor(a_st, a_st + int(rng.integers(0, 900)), 251)
    want = run(ctx, [ref], P.seqs, P.quals)
    stats = ctx.map_stats()
    assert stats[4] >= P.n_pairs, (stats, P.n_pairs)
    skipped = ctx.rescue_skipped()
    assert skipped > 0
    assert skipped >= 100, skipped                        # nearly all of the 120
    assert (want['flag'] & 4 != 0).sum() >= 100           # their mates stay unaligned
    # map_stats()[1] counts the extensions that ran
    ctx.reads_load(P.seqs, P.quals, False)
    ctx.map(_native.params(oracle.E2E))
    assert stats[1] == ctx.map_stats()[1] + stats[4] - skipped


def test_no_skip_other_diagonal_strand_reference(ctx):
    """Nothing but an equal (strand, reference, centre) is skipped: a seed
    cluster one diagonal off the rescue's best (an inserted base next to the
    seed), the same diagonal on the other strand (a reverse-complement
    palindrome), the same diagonal on the other reference of the index."""
    rng = np.random.default_rng(500)
    half = random_ref(rng, M_SKIP // 2)
    pal_at = 1400
    ref = random_ref(rng, pal_at) + half + revcomp(half) + random_ref(rng, 3000 - pal_at - M_SKIP)
    other = list(random_ref(rng, 3000))
    P = Pairs(ref, rng)
    n_indel = n_pal = n_other = 0
    # the seed sits at offset 38 on diagonal b_st, 186 bases after the inserted one on b_st - 1
    for k in range(40):
        a_st = int(rng.integers(100, 850))
        b_st = a_st + int(rng.integers(0, 300))          # ends before the palindrome
        seg = ref[b_st:b_st + M_SKIP]
        x = substituted(seg, 7, 3, keep=[(37, 61)])
        x = x[:62] + 'ACGT'[('ACGT'.index(x[62]) + 2) % 4] + x[62:-1]
        P.add(ref[a_st:a_st + LA], revcomp(x), mate_first=k % 2 == 1)
        n_indel += 1
    # palindrome: the mate as given (strand 0) seeds diagonal pal_at; the anchor is forward, so
    # the rescue looks on strand 1, where the mate fits diagonal pal_at as well
    for k in range(20):
        a_st = int(rng.integers(pal_at - 900, pal_at - LA))
        x = failing_mate(ref[pal_at:pal_at + M_SKIP])
        P.add(ref[a_st:a_st + LA], x, mate_first=k % 2 == 1)
        n_pal += 1
    # other reference: the mate has no exact 22-mer on r0 (rescued there), r1 holds its
    # 22-mer at the same coordinates
    for k in range(20):
        a_st = 100 + 40 * k
        b_st = 1700 + 50 * k                      # past the palindrome; the planted seeds do not overlap
        x = substituted(ref[b_st:b_st + M_SKIP], 15, 7)       # substitutions at 7, 22, ..., 97, 112, ...
        other[b_st + SEED_AT:b_st + SEED_AT + 22] = x[SEED_AT:SEED_AT + 22]
        P.add(ref[a_st:a_st + LA], revcomp(x), mate_first=k % 2 == 1)
        n_other += 1
    want = run(ctx, [ref, ''.join(other)], P.seqs, P.quals, maxins=2600)
    assert ctx.map_stats()[4] >= P.n_pairs, (ctx.map_stats(), P.n_pairs)
    assert ctx.rescue_skipped() == 0
    # the mates of the last group are rescued on r0
    tail = want[-2 * n_other:]
    assert (tail['flag'] & 4 == 0).all() and (tail['ref'] == 0).all()


def test_unpaired_has_no_rescue(ctx):
    rng = np.random.default_rng(600)
    ref = random_ref(rng, 2500)
    P = Pairs(ref, rng)
    for k in range(100):
        a_st = int(rng.integers(100, 1000))
        b_st = a_st + int(rng.integers(0, 900))
        P.add(ref[a_st:a_st + LA], revcomp(failing_mate(ref[b_st:b_st + M_SKIP])))
    run(ctx, [ref], P.seqs, P.quals, paired=False)
    assert ctx.map_stats()[4] == 0
    assert ctx.rescue_skipped() == 0

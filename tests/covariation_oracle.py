"""covariation.csv in plain Python: the specification of the pairwise
covariation of minority variants aln2counts reports (DESIGN.md section 6,
"Covariation"), kept independent of the device pass's method -- strings and
slices, no class codes, no bit columns, no popcounts.

A row's character at a consensus codon in a frame is linkage's
(linkage_oracle._character): one of the 21 letters, '-' (del), '?' (partial),
'X', or none.  The 22 characters of CALLED are *called*; their order in that
string is "character order".

Per run and coordinate position with a consensus codon, tally[ch] is the
summed count of the rows with called character ch and called their sum.  The
major is the character with the largest tally (ties: the earlier one); any
other character with tally >= min_count and tally >= min_fraction * called is
a variant.  More than max_variants: the largest tallies stay, ties by (region
name, position, character order).  The kept ones, ordered by (region name,
position, character order), pair up a < b when their (frame, consensus codon)
differ; over the rows called at both codons n is the summed count, n.a / n.b
those with a's / b's character, n.ab those with both; the pair is written
when n >= min_count.  Only tests import this module.
"""
import io

import amino_detail_oracle as ado
import linkage_oracle as lo
import og_aln2counts as og

CALLED = 'ACDEFGHIKLMNPQRSTVWY*-'
CODES = '\0ACDEFGHIKLMNPQRSTVWY*X?-'          # mh_a2c_gram's code of each character; 0 is blank
CALLED_MASK = sum(1 << CODES.index(ch) for ch in CALLED)
HEADER = ['seed', 'q-cutoff', 'region.a', 'pos.a', 'aa.a', 'region.b', 'pos.b', 'aa.b', 'n', 'n.a', 'n.b',
          'n.ab', 'direction', 'r2']


def _tuples(rows):
    return [(int(r['offset']), r['seq'], int(r['count'])) if isinstance(r, dict) else r for r in rows]


def characters(rows, frame, codon):
    """The character of every row at one consensus codon, None for blank."""
    return [lo._character('-' * (frame + offset) + seq, frame + offset, len(seq), codon)
            for offset, seq, _n in _tuples(rows)]


def gram(rows, cols):
    """What Context.a2c_gram returns for cols = [(frame, codon, mask)]: per
    pair of columns the summed count of the rows both hold, as lists."""
    rows = _tuples(rows)
    seen = {}
    out = [[0] * len(cols) for _ in cols]
    for frame, codon, _mask in cols:
        if (frame, codon) not in seen:
            seen[frame, codon] = characters(rows, frame, codon)
    for r, (_offset, _seq, count) in enumerate(rows):
        held = [i for i, (frame, codon, mask) in enumerate(cols)
                if seen[frame, codon][r] is not None and mask >> CODES.index(seen[frame, codon][r]) & 1]
        for i in held:
            for j in held:
                out[i][j] += count
    return out


def direction(n, na, nb, nab):
    return '+' if n * nab > na * nb else '-' if n * nab < na * nb else '0'


def r2(n, na, nb, nab):
    """'%.4f' of the squared correlation of the two indicators, '' when a
    margin is empty or full."""
    bottom = na * (n - na) * nb * (n - nb)
    return '' if bottom == 0 else '%.4f' % ((n * nab - na * nb) ** 2 / bottom)


def select(tallies, min_fraction, min_count, max_variants):
    """tallies: {(region, position): {called character: summed count}} of one
    run.  ([(region, position, character)] kept, in pair order; dropped)."""
    found = []
    for (region, pos), tally in tallies.items():
        called = sum(tally.values())
        if not called:
            continue
        major = max(CALLED, key=lambda ch: (tally.get(ch, 0), -CALLED.index(ch)))
        for ch in CALLED:
            t = tally.get(ch, 0)
            if ch != major and t >= min_count and t >= min_fraction * called:
                found.append((-t, region, pos, CALLED.index(ch)))
    found.sort()
    kept = sorted(v[1:] for v in found[:max_variants])
    return [(region, pos, CALLED[c]) for region, pos, c in kept], len(found) - len(kept)


def pairs(rows, variants, place, min_count):
    """The records of one run: variants = [(region, position, character)] in
    pair order, place = {(region, position): (frame, consensus codon)}.
    [(region.a, pos.a, aa.a, region.b, pos.b, aa.b, n, n.a, n.b, n.ab)]."""
    rows = _tuples(rows)
    chars = {}
    for region, pos, _ch in variants:
        site = place[region, pos]
        if site not in chars:
            chars[site] = characters(rows, *site)
    out = []
    for i, a in enumerate(variants):
        for b in variants[i + 1:]:
            sa, sb = place[a[0], a[1]], place[b[0], b[1]]
            if sa == sb:
                continue
            n = na = nb = nab = 0
            for (_o, _s, count), x, y in zip(rows, chars[sa], chars[sb]):
                if x is None or y is None or x not in CALLED or y not in CALLED:
                    continue
                n += count
                na += count * (x == a[2])
                nb += count * (y == b[2])
                nab += count * (x == a[2] and y == b[2])
            if n >= min_count:
                out.append(a + b + (n, na, nb, nab))
    return out


def line(seed, qcut, record):
    n, na, nb, nab = record[6:]
    return [seed, qcut] + [str(x) for x in record] + [direction(n, na, nb, nab), r2(n, na, nb, nab)]


def run_tallies(rep, group):
    """({(region, position): tally}, {(region, position): (frame, codon)}) of
    the run the oracle Report has just read: the regions a frame aligned to,
    the positions with a consensus codon."""
    rows = _tuples(group)
    tallies, place, by_site = {}, {}, {}
    for region in sorted(rep.reports):
        if not rep.reports[region]:
            continue
        frame = rep.reading_frames[region]
        for t, pos in rep.reports[region]:
            k = t.consensus_index
            if k is None:
                continue
            if (frame, k) not in by_site:
                tally = {}
                for (_o, _s, count), ch in zip(rows, characters(rows, frame, k)):
                    if ch is not None and ch in CALLED:
                        tally[ch] = tally.get(ch, 0) + count
                by_site[frame, k] = tally
            tallies[region, pos] = by_site[frame, k]
            place[region, pos] = (frame, k)
    return tallies, place


def expected(aligned_text, min_fraction=0.01, min_count=10, max_variants=256):
    """(rows of covariation.csv without the header, [per run (seed, q-cutoff,
    variants kept, dropped, records)]): runs in file order."""
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    lines, runs = [], []
    translate, seen = og.translate, {}

    def memo(*args):          # Report.read translates every codon of every row anew
        if args not in seen:
            seen[args] = translate(*args)
        return seen[args]
    og.translate = memo
    try:
        for group in ado.groups(aligned_text):
            rep.read(group)
            tallies, place = run_tallies(rep, group)
            kept, dropped = select(tallies, min_fraction, min_count, max_variants)
            records = pairs(group, kept, place, min_count)
            runs.append((rep.seed, rep.qcut, kept, dropped, records))
            lines.extend(line(rep.seed, rep.qcut, r) for r in records)
    finally:
        og.translate = translate
    return lines, runs

"""linkage.csv in plain Python: the specification of the linked amino acids
aln2counts counts at chosen positions ("Linked amino
acids"), kept independent of the device pass's method -- strings and slices,
no class codes, no bins, no keys.

A set is 1 to 12 strictly increasing 1-based amino-acid positions of one
coordinate region.  In a run the region has a reading frame f and a consensus
codon k per position (none: the set is unplaced and writes nothing).  For a
row (offset, seq, count) the codon at k is characters 3k .. 3k + 2 of
'-' * (f + offset) + seq, '-' past either end; its class is
amino_detail_oracle.classify's and its character

    letter   the letter (translate of the upper-cased codon, '*' included)
    del      '-'
    partial  '?'
    X        'X'
    blank    none: the row does not count for the set

A row counts for a set when none of the set's codons is blank; its haplotype
is the set's characters in the set's order; equal haplotypes add their counts
up; coverage is the summed count of every row that counts.  The rows of the
file are the haplotypes with count >= min_count by count descending, then
haplotype (as bytes) ascending.  Only tests import this module.
"""
import io

import amino_detail_oracle as ado
import og_aln2counts as og

HEADER = ['seed', 'region', 'q-cutoff', 'positions', 'haplotype', 'count', 'coverage']
_CHAR = {'del': '-', 'partial': '?', 'X': 'X'}


def _character(padded, lead, n, k):
    """The haplotype character of consensus codon k of a row of n bytes behind
    lead characters of padding, None for a blank codon."""
    codon = padded[3 * k:3 * k + 3]
    codon += '-' * (3 - len(codon))
    inside = tuple(lead <= p < lead + n for p in range(3 * k, 3 * k + 3))
    kind = ado.classify(codon, inside)
    if kind == 'blank':
        return None
    if kind == 'letter':
        return og.translate(codon.upper())
    return _CHAR[kind]


def haplotype(offset, seq, frame, codons):
    """The row's haplotype over the consensus codons, None when it does not
    count."""
    padded = '-' * (frame + offset) + seq
    chars = [_character(padded, frame + offset, len(seq), k) for k in codons]
    return None if None in chars else ''.join(chars)


def count(rows, frame, codons):
    """({haplotype: summed count}, coverage) of one placed set over a group's
    rows (dicts or (offset, seq, count) tuples)."""
    found, coverage = {}, 0
    for row in rows:
        if isinstance(row, dict):
            row = int(row['offset']), row['seq'], int(row['count'])
        offset, seq, n = row
        hap = haplotype(offset, seq, frame, codons)
        if hap is not None:
            found[hap] = found.get(hap, 0) + n
            coverage += n
    return found, coverage


def ordered(found, min_count=1):
    """[(haplotype, count)] of a set in report order."""
    return sorted(((h, n) for h, n in found.items() if n >= min_count),
                  key=lambda e: (-e[1], e[0].encode()))


def entries(rows, sets, min_count=1):
    """What Context.a2c_link returns for sets = [(frame, [codons])]:
    ([(set index, count, haplotype bytes)], [coverage per set])."""
    out, coverage = [], []
    for s, (frame, codons) in enumerate(sets):
        found, cov = count(rows, frame, codons)
        coverage.append(cov)
        out.extend((s, n, h.encode()) for h, n in ordered(found, min_count))
    return out, coverage


def place(report, region, positions):
    """(frame, [consensus codon per position]) of a set in the oracle Report's
    map of a region it has read, None when a position has no codon."""
    by_pos = {pos: t.consensus_index for t, pos in report.reports[region]}
    codons = [by_pos.get(p) for p in positions]
    if None in codons:
        return None
    return report.reading_frames[region], codons


def expected(aligned_text, positions, min_count=1):
    """(rows of linkage.csv without the header, [(seed, q-cutoff, region, set
    index)] of the unplaced sets, {(seed, q-cutoff, region, set index):
    ({haplotype: count}, coverage)}): runs in file order, regions in name
    order, sets in the order given."""
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    lines, unplaced, tallies = [], [], {}
    translate, seen = og.translate, {}

    def memo(*args):          # Report.read translates every codon of every row anew
        if args not in seen:
            seen[args] = translate(*args)
        return seen[args]
    og.translate = memo
    try:
        for group in ado.groups(aligned_text):
            rep.read(group)
            for region in sorted(positions):
                if not rep.reports.get(region):      # not a region of the seed, or no frame aligned
                    continue
                for s, chosen in enumerate(positions[region]):
                    placed = place(rep, region, chosen)
                    if placed is None:
                        unplaced.append((rep.seed, rep.qcut, region, s))
                        continue
                    found, coverage = count(group, *placed)
                    tallies[rep.seed, rep.qcut, region, s] = found, coverage
                    lines.extend([rep.seed, region, rep.qcut, ';'.join(str(p) for p in chosen), h, str(n),
                                  str(coverage)] for h, n in ordered(found, min_count))
    finally:
        og.translate = translate
    return lines, unplaced, tallies

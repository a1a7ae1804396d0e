"""amino_detail.csv in plain Python: the specification of the codon classes
aln2counts counts beside amino.csv's 21 letters ("Codon
classes"), kept independent of the device pass's method -- strings and
slices, no class codes, no bins.

For a row (offset, seq, count) of an aligned.csv group and a reading frame f
in 0..2 the padded text is '-' * (f + offset) + seq, padded with '-' to a
codon boundary, and the codons looked at are j = offset // 3 ..
len(padded) // 3 - 1: the ones the reference's _count_reads visits
(aln2counts.py:155-169).  Each of a codon's three characters is a base
(A C G T N), a '-' inside (an index of seq), a '-' outside (padding) or 'n',
the gap between mates.  With a = translate(codon.upper()):

    letter   a is one of the 21 letters: amino.csv's own, no new class
    del      all three characters are '-' inside
    blank    none of the three is a base: counted nowhere
    partial  at least one is '-' (inside or outside) or 'n'
    X        otherwise: three of A C G T N with an ambiguous translation

the first that applies; each adds the row's count at (frame, codon).
amino_detail.csv is amino.csv's rows followed by X, partial, del, ins, clip,
coverage (expected_rows).  Only tests import this module.
"""
import csv
import io
import itertools

import og_aln2counts as og

CLASSES = ('X', 'partial', 'del')
HEADER = (['seed', 'region', 'q-cutoff', 'query.aa.pos', 'refseq.aa.pos'] + list(og.AMINOS) +
          ['X', 'partial', 'del', 'ins', 'clip', 'coverage'])
_AMINO = {}
_CLASS = {}
_ALL = (True, True, True)


def _amino(codon):
    if codon not in _AMINO:
        _AMINO[codon] = og.translate(codon.upper())
    return _AMINO[codon]


def codons(offset, seq, frame):
    """[(codon index, codon text, inside flags)] of one row in one frame."""
    lead = frame + offset
    padded = '-' * lead + seq
    padded += '-' * (-len(padded) % 3)
    out = []
    for j in range(offset // 3, len(padded) // 3):
        if lead <= 3 * j and 3 * j + 3 <= lead + len(seq):
            inside = _ALL
        else:
            inside = tuple(lead <= p < lead + len(seq) for p in range(3 * j, 3 * j + 3))
        out.append((j, padded[3 * j:3 * j + 3], inside))
    return out


def classify(codon, inside):
    """'letter', 'del', 'blank', 'partial' or 'X' of one codon."""
    if (codon, inside) not in _CLASS:
        _CLASS[codon, inside] = _classify(codon, inside)
    return _CLASS[codon, inside]


def _classify(codon, inside):
    if _amino(codon) in og.AMINOS:
        return 'letter'
    if all(ch == '-' and within for ch, within in zip(codon, inside)):
        return 'del'
    if not any(ch in 'ACGTN' for ch in codon):
        return 'blank'
    if any(ch in '-n' for ch in codon):
        return 'partial'
    return 'X'


def tally(rows):
    """{(frame, codon): {class: summed count}} of a group's rows (dicts or
    (offset, seq, count) tuples), 'letter' and 'blank' included."""
    out = {}
    for row in rows:
        if isinstance(row, dict):
            row = int(row['offset']), row['seq'], int(row['count'])
        offset, seq, count = row
        for frame in range(3):
            for j, codon, inside in codons(offset, seq, frame):
                cell = out.setdefault((frame, j), {})
                k = classify(codon, inside)
                cell[k] = cell.get(k, 0) + count
    return out


def table(rows, frame, ncod):
    """[[X, partial, del]] of codons 0 .. ncod - 1 of one frame."""
    cells = tally(rows)
    return [[cells.get((frame, j), {}).get(k, 0) for k in CLASSES] for j in range(ncod)]


def groups(aligned_text):
    """The (refname, qcut) runs of aligned.csv text, as lists of row dicts."""
    return [list(g) for _key, g in itertools.groupby(csv.DictReader(io.StringIO(aligned_text)),
                                                     lambda r: (r['refname'], r['qcut']))]


def expected_rows(aligned_text, clips=None, ins=None):
    """(rows of amino_detail.csv without the header, reading frame of each):
    the oracle Report's write_amino_counts walk, then per row X, partial and
    del of the row's consensus codon in the region's frame, ins, clip and
    coverage.  With k = query.aa.pos - 1 and f the region's frame the codon
    is consensus positions p = 3k - f + 1 .. 3k - f + 3: ins is the sum over
    them of ins[(seed, qcut, p)] ({} entries of ins_oracle.totals), clip the
    largest clips[(seed, p)] (clip_oracle.as_dict); '' for a column whose
    input is None, 0 without a query position."""
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    rows, frames = [], []
    translate, seen = og.translate, {}

    def memo(*args):          # Report.read translates every codon of every row anew
        if args not in seen:
            seen[args] = translate(*args)
        return seen[args]
    og.translate = memo
    try:
        for group in groups(aligned_text):
            rep.read(group)
            cells = tally(group)
            for region in sorted(rep.reports):
                f = rep.reading_frames.get(region, 0)
                for t, pos in rep.reports[region]:
                    k = t.consensus_index
                    letters = [t.counts[a] for a in og.AMINOS]
                    if k is None:
                        xpd, p = [0, 0, 0], []
                    else:
                        xpd = [cells.get((f, k), {}).get(c, 0) for c in CLASSES]
                        p = [3 * k - f + 1 + t3 for t3 in range(3)]
                    n_ins = '' if ins is None else sum(ins.get((rep.seed, int(rep.qcut), q), 0) for q in p)
                    clip = '' if clips is None else max([clips.get((rep.seed, q), 0) for q in p] or [0])
                    rows.append([str(x) for x in [rep.seed, region, rep.qcut, '' if k is None else k + 1, pos] +
                                 letters + xpd + [n_ins, clip, sum(letters) + sum(xpd)]])
                    frames.append(f)
    finally:
        og.translate = translate
    return rows, frames

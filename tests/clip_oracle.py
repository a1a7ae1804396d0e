"""clipping.csv in plain Python: the specification of sam2aln's soft-clip
counts ("Soft-clip counts"), kept independent of the
device pass's method -- sets of positions per read, no interval sweep.

A unit of og_sam2aln.matchmaker counts when it reaches the merge: its cause
in failed.csv is none of unmatched, badCigar, 2refs (a manyNs pair counts).
Per read with 1-based POS p:

    lead    = the S ops before the first op that is not S
    trail   = every other S op
    span    = M + D
    clipped = {p - lead .. p - 1} | {p + span .. p + span + trail - 1}
    mapped  = {p .. p + span - 1}

and the unit adds 1 to every position of (clipped1 | clipped2) - (mapped1 |
mapped2) of its reference.  Only tests import this module.
"""
import csv
import io

import og_sam2aln

NOT_MERGED = ('unmatched', 'badCigar', '2refs')


def read_sets(row):
    """(clipped, mapped) position sets of one remap.csv row."""
    p = int(row['pos'])
    ops = [(int(n), op) for n, op in og_sam2aln._TOKEN.findall(row['cigar'])]
    k = 0
    while k < len(ops) and ops[k][1] == 'S':
        k += 1
    lead = sum(n for n, _ in ops[:k])
    trail = sum(n for n, op in ops[k:] if op == 'S')
    span = sum(n for n, op in ops if op in 'MD')
    clipped = set(range(p - lead, p)) | set(range(p + span, p + span + trail))
    mapped = set(range(p, p + span))
    return clipped, mapped


def unit_sets(row1, row2):
    """The (clipped, mapped) sets of the reads a unit merges, or None when
    the unit does not reach the merge."""
    _, _, _, failed = og_sam2aln.parse_sam(row1, row2)
    if any(f['cause'] in NOT_MERGED for f in failed):
        return None
    paired = int(row1['flag']) & 1
    return [read_sets(row) for row in ((row1, row2) if paired else (row1,))]


def clipping(remap_text):
    """(clipping.csv text, tallies) of remap.csv text.  tallies counts the
    units by class: 'units' that reach the merge, 'contributing' ones with at
    least one counted position, 'lost_to_mate' pairs with a position one mate
    clips and the other aligns, 'common' pairs whose mates clip a common
    position."""
    counts = {}
    tallies = dict(units=0, contributing=0, lost_to_mate=0, common=0)
    for row1, row2 in og_sam2aln.matchmaker(csv.DictReader(io.StringIO(remap_text))):
        sets = unit_sets(row1, row2)
        if sets is None:
            continue
        tallies['units'] += 1
        clipped = set().union(*(c for c, _ in sets))
        mapped = set().union(*(m for _, m in sets))
        if len(sets) == 2:
            tallies['lost_to_mate'] += bool(clipped & mapped)
            tallies['common'] += bool(sets[0][0] & sets[1][0])
        kept = clipped - mapped
        tallies['contributing'] += bool(kept)
        ref = counts.setdefault(row1['rname'], {})
        for pos in kept:
            ref[pos] = ref.get(pos, 0) + 1
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(['refname', 'pos', 'count'])
    for rname in sorted(counts):
        for pos in sorted(counts[rname]):
            w.writerow([rname, pos, counts[rname][pos]])
    return out.getvalue(), tallies


def as_dict(clipping_text):
    """{(refname, pos): count} of clipping.csv text."""
    return {(r['refname'], int(r['pos'])): int(r['count'])
            for r in csv.DictReader(io.StringIO(clipping_text))}

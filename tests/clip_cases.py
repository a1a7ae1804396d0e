"""Hand-written remap.csv texts for sam2aln's soft-clip counts, with the
clipping.csv each must give worked out by hand from the rule (DESIGN.md
section 6, "Soft-clip counts"): tests/test_clip_oracle.py holds the oracle to
them, tests/test_gpu_clipping.py the device pass."""
import csv
import io
import re

HEADER = ['qname', 'flag', 'rname', 'pos', 'mapq', 'cigar', 'rnext', 'pnext', 'tlen', 'seq', 'qual']
FWD, REV, UNPAIRED = 99, 147, 0


def row(qname, flag, rname, pos, cigar, qual='I'):
    """One remap.csv row: SEQ / QUAL as long as the CIGAR's read bases."""
    n = sum(int(k) for k, op in re.findall(r'(\d+)([MIS])', cigar)) if cigar != '*' else 4
    return [qname, flag, rname, pos, 44, cigar, '=', pos, 0, ('ACGT' * n)[:n], qual * n]


def text(rows):
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows(rows)
    return out.getvalue()


def expected_text(counts):
    """clipping.csv of {(refname, pos): count}."""
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(['refname', 'pos', 'count'])
    w.writerows([r, p, counts[r, p]] for r, p in sorted(counts))
    return out.getvalue()


def _span(ref, lo, hi, n=1):
    return {(ref, p): n for p in range(lo, hi + 1)}


# name -> (rows, {(refname, pos): count})
CASES = {
    # 3S5M at 10: the three bases before POS
    'lead_only': ([row('a', UNPAIRED, 'R1', 10, '3S5M')], _span('R1', 7, 9)),
    # 5M2S at 10: aligned 10..14, clipped 15, 16
    'trail_only': ([row('a', UNPAIRED, 'R1', 10, '5M2S')], _span('R1', 15, 16)),
    # two S ops before the first other op are both the lead: 5..9
    'split_lead': ([row('a', UNPAIRED, 'R1', 10, '3S2S5M')], _span('R1', 5, 9)),
    # lead and trail around a deletion and an insertion: span = 4 + 2 + 3
    'both_ends': ([row('a', UNPAIRED, 'R1', 100, '2S4M2D1I3M3S')],
                  {**_span('R1', 98, 99), **_span('R1', 109, 111)}),
    # a read that is all S has no other op: all of it is lead, 16..19; its
    # mate aligns 30..35
    'all_s': ([row('a', FWD, 'R1', 20, '4S'), row('a', REV, 'R1', 30, '6M')], _span('R1', 16, 19)),
    # the mate aligns 5..12, over the 7..9 the first read clips
    'mate_covers': ([row('a', FWD, 'R1', 10, '3S5M'), row('a', REV, 'R1', 5, '8M')], {}),
    # the mate aligns 8..12: of the clipped 6..9 only 6, 7 are left, and its
    # own trail 13, 14 lies inside the first read's 10..14
    'mate_covers_part': ([row('a', FWD, 'R1', 10, '4S5M'), row('a', REV, 'R1', 8, '5M2S')],
                         _span('R1', 6, 7)),
    # both mates clip 8, 9: the unit counts once
    'both_clip': ([row('a', FWD, 'R1', 10, '2S5M'), row('a', REV, 'R1', 10, '2S6M')],
                  _span('R1', 8, 9)),
    # POS 2 with five clipped bases: -3..1
    'below_one': ([row('a', UNPAIRED, 'R1', 2, '5S4M')], _span('R1', -3, 1)),
    # references in file order zeta, then 'b,1' (quoted in both files), then
    # alpha; two units on zeta
    'two_refs': ([row('a', UNPAIRED, 'zeta', 10, '1S5M'), row('b', UNPAIRED, 'b,1', 7, '4M2S'),
                  row('c', UNPAIRED, 'alpha', 50, '2S5M'), row('d', UNPAIRED, 'zeta', 9, '2S5M1S')],
                 {('alpha', 48): 1, ('alpha', 49): 1, ('b,1', 11): 1, ('b,1', 12): 1,
                  ('zeta', 7): 1, ('zeta', 8): 1, ('zeta', 9): 1, ('zeta', 14): 1}),
    # unmatched (a paired flag and no mate), badCigar ('*'), 2refs: not counted
    'unmatched': ([row('a', FWD, 'R1', 10, '2S4M')], {}),
    'bad_cigar': ([row('a', FWD, 'R1', 10, '2S4M'), row('a', REV, 'R1', 10, '*')], {}),
    'two_refs_pair': ([row('a', FWD, 'R1', 10, '2S4M'), row('a', REV, 'R2', 10, '2S4M')], {}),
    # every base below the cutoff: manyNs in failed.csv, counted all the same
    'many_ns': ([row('a', FWD, 'R1', 10, '2S6M', '#'), row('a', REV, 'R1', 10, '2S6M', '#')],
                _span('R1', 8, 9)),
}
FAILED_CAUSE = {'unmatched': 'unmatched', 'bad_cigar': 'badCigar', 'two_refs_pair': '2refs',
                'many_ns': 'manyNs'}


def combined():
    """Every case in one text (qnames made distinct): the counts add up."""
    rows, counts = [], {}
    for name, (case_rows, want) in CASES.items():
        rows += [[name + '.' + r[0]] + r[1:] for r in case_rows]
        for key, n in want.items():
            counts[key] = counts.get(key, 0) + n
    return rows, counts

"""concordance.csv and cycle_concordance.csv in plain Python: the
specification of sam2aln's mate concordance ("Mate
concordance"), kept independent of the device pass's method -- a dict of
positions per read, no interval arithmetic, no difference array.

A unit of og_sam2aln.matchmaker counts when it reaches the merge (its cause in
failed.csv is none of unmatched, badCigar, 2refs; a manyNs pair counts) and
row 1's flag has bit 1.  Each mate is expanded as apply_cigar expands it, with
1-based POS p: an M op puts the read's (byte, quality byte, read index) at
consecutive positions from p, a D op puts ('-', ' ', None), I and S ops only
advance the read index.

Per position y both mates hold: overlap += 1; when the bytes differ, one of
nocall (either is 'N'), indel (either is '-'), mismatch += 1, and unresolved
+= 1 when the quality bytes are closer than 5.

Per read: where both mates have a read index and neither byte is 'N', each
mate adds 1 to compared -- and to mismatch when the bytes differ -- at
(read, 'cycle', cycle) and (read, 'quality', quality byte - 33); read is 1
with flag 0x40, else 2; cycle is index + 1, or len(seq) - index with flag
0x10.  Only tests import this module.
"""
import csv
import io

import og_sam2aln

NOT_MERGED = ('unmatched', 'badCigar', '2refs')
POSITION_HEADER = ['refname', 'pos', 'overlap', 'mismatch', 'indel', 'nocall', 'unresolved']
READ_HEADER = ['read', 'by', 'value', 'compared', 'mismatch']
MINIMUM_Q_DELTA = 5


def expand(row):
    """{position: (byte, quality byte, read index or None)} of one row."""
    y = int(row['pos'])
    x = 0
    seq, qual = row['seq'], row['qual']
    out = {}
    for n, op in og_sam2aln._TOKEN.findall(row['cigar']):
        for _ in range(int(n)):
            if op == 'M':
                out[y] = seq[x], qual[x], x
                x += 1
                y += 1
            elif op == 'D':
                out[y] = '-', ' ', None
                y += 1
            else:                       # I, S
                x += 1
    return out


def _read_keys(row, x, q):
    flag = int(row['flag'])
    read = 1 if flag & 0x40 else 2
    cycle = len(row['seq']) - x if flag & 0x10 else x + 1
    return (read, 'cycle', cycle), (read, 'quality', ord(q) - 33)


def count(remap_text):
    """(positions, reads) of remap.csv text: positions = {(refname, pos):
    [overlap, mismatch, indel, nocall, unresolved]}, reads = {(read, by,
    value): [compared, mismatch]}."""
    positions, reads = {}, {}
    for row1, row2 in og_sam2aln.matchmaker(csv.DictReader(io.StringIO(remap_text))):
        _, _, _, failed = og_sam2aln.parse_sam(row1, row2)
        if any(f['cause'] in NOT_MERGED for f in failed):
            continue
        if not int(row1['flag']) & 1:
            continue
        e1, e2 = expand(row1), expand(row2)
        for y in e1:
            if y not in e2:
                continue
            (c1, q1, x1), (c2, q2, x2) = e1[y], e2[y]
            at = positions.setdefault((row1['rname'], y), [0, 0, 0, 0, 0])
            at[0] += 1
            if c1 != c2:
                at[3 if 'N' in (c1, c2) else 2 if '-' in (c1, c2) else 1] += 1
                if abs(ord(q1) - ord(q2)) < MINIMUM_Q_DELTA:
                    at[4] += 1
            if x1 is None or x2 is None or 'N' in (c1, c2):
                continue
            for key in _read_keys(row1, x1, q1) + _read_keys(row2, x2, q2):
                cell = reads.setdefault(key, [0, 0])
                cell[0] += 1
                cell[1] += c1 != c2
    return positions, reads


def position_text(positions):
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(POSITION_HEADER)
    w.writerows([name, pos] + positions[name, pos] for name, pos in sorted(positions))
    return out.getvalue()


def read_text(reads):
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(READ_HEADER)
    w.writerows(list(key) + reads[key] for key in sorted(reads))
    return out.getvalue()


def concordance(remap_text):
    """(concordance.csv text, cycle_concordance.csv text) of remap.csv text."""
    positions, reads = count(remap_text)
    return position_text(positions), read_text(reads)


def position_dict(text):
    """{(refname, pos): [overlap, mismatch, indel, nocall, unresolved]} of concordance.csv text."""
    return {(r['refname'], int(r['pos'])): [int(r[k]) for k in POSITION_HEADER[2:]]
            for r in csv.DictReader(io.StringIO(text))}


def read_dict(text):
    """{(read, by, value): [compared, mismatch]} of cycle_concordance.csv text."""
    return {(int(r['read']), r['by'], int(r['value'])): [int(r['compared']), int(r['mismatch'])]
            for r in csv.DictReader(io.StringIO(text))}

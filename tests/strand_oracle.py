"""strand.csv in plain Python: the specification of sam2aln's strand support
("Strand support"), built on og_sam2aln's matchmaker,
parse_sam and merge_pairs and kept independent of the device pass's method --
no classes of cutoffs, no windows: every cutoff's merged string is walked
against each mate's own expansion.

A unit of og_sam2aln.matchmaker counts at the cutoffs at which parse_sam
gives it a merged string (none with cause unmatched, badCigar or 2refs, none
at a cutoff where it is manyNs).  mseq is that string; index j is position
y = j + 1.  Only m = mseq[j] in 'ACGT-' counts.  A mate supports m at y when
its expansion -- apply_cigar's string behind max(POS - 1, 0) bytes of padding,
which support nothing -- holds the byte m at index j; the mate is 'rev' with
FLAG 0x10, else 'fwd'.  Per unit, cutoff, y and m: m_fwd += 1 if a supporting
mate is forward, m_rev += 1 if one is reversed, m_both += 1 if both hold.

The strings are compared as byte arrays (numpy) so that a golden takes a few
seconds.  Only tests import this module.
"""
import csv
import io

import numpy as np

import og_sam2aln

BASES = 'ACGT-'
NAMES = ('A', 'C', 'G', 'T', 'del')
HEADER = ['refname', 'qcut', 'pos'] + [n + s for n in NAMES for s in ('_fwd', '_rev', '_both')]
_CODE = np.full(256, 5, dtype=np.int64)
for _k, _c in enumerate(BASES):
    _CODE[ord(_c)] = _k


def _bytes(s):
    return np.frombuffer(s.encode('latin-1'), dtype=np.uint8)


def count(remap_text, cuts=(15,)):
    """{(refname, qcut, pos): [15 counts in HEADER's order]} of remap.csv text
    at the cutoffs `cuts`; only keys with a count above 0."""
    cuts = list(cuts)
    planes = {}                          # (refname, qcut) -> int64 [24, positions]: code * 4 + fwd + 2 * rev
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = cuts
    try:
        for row1, row2 in og_sam2aln.matchmaker(csv.DictReader(io.StringIO(remap_text))):
            rname, mseqs, _, _ = og_sam2aln.parse_sam(row1, row2)
            if not mseqs:
                continue
            mates = []
            for row in (row1, row2) if int(row1['flag']) & 1 else (row1,):
                s = og_sam2aln.apply_cigar(row['cigar'], row['seq'], row['qual'])[0]
                pad = max(int(row['pos']) - 1, 0)
                mates.append((np.concatenate([np.zeros(pad, dtype=np.uint8), _bytes(s)]),
                              bool(int(row['flag']) & 0x10)))
            for qcut, mseq in mseqs.items():
                m = _bytes(mseq)
                n = len(m)
                sup = np.zeros(n, dtype=np.int64)
                for exp, rev in mates:
                    k = min(n, len(exp))
                    sup[:k] |= (exp[:k] == m[:k]) * (2 if rev else 1)
                hist = np.bincount((_CODE[m] * 4 + sup) * n + np.arange(n), minlength=24 * n).reshape(24, n)
                old = planes.get((rname, qcut))
                if old is None or old.shape[1] < n:
                    grown = np.zeros((24, max(n, 2 * (0 if old is None else old.shape[1]))), dtype=np.int64)
                    if old is not None:
                        grown[:, :old.shape[1]] = old
                    planes[rname, qcut] = old = grown
                old[:, :n] += hist
    finally:
        og_sam2aln.Q_CUTOFFS = saved
    out = {}
    for (rname, qcut), p in planes.items():
        cols = []
        for k in range(5):
            fwd_only, rev_only, both = p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]
            cols += [fwd_only + both, rev_only + both, both]
        table = np.stack(cols, axis=1)
        for j in np.flatnonzero(table.any(axis=1)).tolist():
            out[rname, qcut, j + 1] = table[j].tolist()
    return out


def text(counts, cuts=(15,)):
    """strand.csv of count()'s result: references as Python sorts str, the
    cutoffs in the order given, positions ascending."""
    cuts = list(cuts)
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows([name, q, pos] + counts[name, q, pos]
                for name, q, pos in sorted(counts, key=lambda k: (k[0], cuts.index(k[1]), k[2])))
    return out.getvalue()


def strand(remap_text, cuts=(15,)):
    """strand.csv text of remap.csv text."""
    return text(count(remap_text, cuts), cuts)


def rows(strand_text):
    """{(refname, qcut, pos): [15 counts]} of strand.csv text."""
    return {(r['refname'], int(r['qcut']), int(r['pos'])): [int(r[k]) for k in HEADER[3:]]
            for r in csv.DictReader(io.StringIO(strand_text))}


def called(counts):
    """{(refname, qcut, pos): [A, C, G, T, del]}: fwd + rev - both of every
    base, the units that call it; keys with any above 0."""
    out = {}
    for key, v in counts.items():
        five = [v[3 * k] + v[3 * k + 1] - v[3 * k + 2] for k in range(5)]
        if any(five):
            out[key] = five
    return out


def aligned_calls(aligned_text):
    """{(refname, qcut, pos): [A, C, G, T, del]} of aligned.csv text: the sum
    of count over the rows whose seq holds the base at pos - 1 - offset."""
    planes = {}
    for r in csv.DictReader(io.StringIO(aligned_text)):
        key = r['refname'], int(r['qcut'])
        m = _bytes(r['seq'])
        off, n = int(r['offset']), len(m)
        hist = np.bincount(_CODE[m] * n + np.arange(n), minlength=6 * n).reshape(6, n)[:5] * int(r['count'])
        old = planes.get(key)
        if old is None or old.shape[1] < off + n:
            grown = np.zeros((5, max(off + n, 2 * (0 if old is None else old.shape[1]))), dtype=np.int64)
            if old is not None:
                grown[:, :old.shape[1]] = old
            planes[key] = old = grown
        old[:, off:off + n] += hist
    out = {}
    for (name, q), p in planes.items():
        for j in np.flatnonzero(p.any(axis=0)).tolist():
            out[name, q, j + 1] = p[:, j].tolist()
    return out

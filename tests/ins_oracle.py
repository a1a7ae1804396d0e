"""conseq_ins.csv in plain Python: the specification of sam2aln's merged
insertions ("Merged insertions").

A unit of og_sam2aln.matchmaker counts at q-cutoff c when it contributes a
sequence to aligned.csv at c: it reaches the merge (its cause is none of
unmatched, badCigar, 2refs) and its merged sequence at c is not manyNs.
Mate 1 is the unit's first row, mate 2 its second (none for an unpaired
unit).  Per read, walking the CIGAR with ref = POS - 1 and left = 0 (M
advances both, D ref, S and I left), an I op of n > 0 bases records

    ins[ref] = (seq[left:left + n], qual[left:left + n])

a later I op with the same key replacing the earlier one.  The key is the
0-based consensus coordinate of the base that follows the insertion -- not
insert.csv's pos, which is a read offset.  Per cutoff the unit's strings are
merge_inserts(ins1, ins2, c) (sam2aln.py:240-273, restated below), and
conseq_ins.csv counts the units per (reference, cutoff, key, string).  An
inserted '-' is refused (Refused, naming the read).  Only tests import this
module.
"""
import csv
import io

import og_sam2aln

NOT_MERGED = ('unmatched', 'badCigar', '2refs')
HEADER = ['refname', 'qcut', 'pos', 'insert', 'count']


class Refused(Exception):
    """A read whose inserted bases hold a '-'; args[0] is its qname."""


def merge_inserts(ins1, ins2, q_cutoff=10, minimum_q_delta=5):
    """{key: merged string} of two {key: (seq, qual)} (None: no insertions)."""
    ins1 = {} if ins1 is None else ins1
    ins2 = {} if ins2 is None else ins2
    cut = chr(q_cutoff + 33)
    merged = {key: seq for key, (seq, qual) in ins1.items() if min(qual) > cut}
    for key, (seq2, qual2) in ins2.items():
        if min(qual2) > cut:
            seq1, qual1 = ins1.get(key, ('', ''))
            merged[key] = og_sam2aln.merge_pairs(seq1, seq2, qual1, qual2, q_cutoff=q_cutoff,
                                                 minimum_q_delta=minimum_q_delta)
    return merged


def read_insertions(row):
    """{key: (seq, qual)} of one remap.csv row."""
    ref, left, ins = int(row['pos']) - 1, 0, {}
    for n, op in og_sam2aln._TOKEN.findall(row['cigar']):
        n = int(n)
        if op == 'M':
            ref += n
            left += n
        elif op == 'D':
            ref += n
        elif op == 'S':
            left += n
        elif op == 'I':
            if n > 0:
                ins[ref] = (row['seq'][left:left + n], row['qual'][left:left + n])
            left += n
    return ins


def units(remap_text, q_cutoffs=(15,)):
    """Per unit that reaches the merge: (rname, the cutoffs at which it
    contributes to aligned.csv, ins1, ins2)."""
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = list(q_cutoffs)
    try:
        for row1, row2 in og_sam2aln.matchmaker(csv.DictReader(io.StringIO(remap_text))):
            rname, mseqs, _, failed = og_sam2aln.parse_sam(row1, row2)
            if any(f['cause'] in NOT_MERGED for f in failed):
                continue
            mates = (row1, row2) if int(row1['flag']) & 1 else (row1,)
            ins = [read_insertions(row) for row in mates] + [{}]
            for per_read in ins:
                if any('-' in seq for seq, _ in per_read.values()):
                    raise Refused(row1['qname'])
            yield rname, sorted(mseqs), ins[0], ins[1]
    finally:
        og_sam2aln.Q_CUTOFFS = saved


def counts(remap_text, q_cutoffs=(15,)):
    """({(refname, qcut, key, string): units}, tallies): tallies counts the
    'insertions' (unit x key x cutoff that gave a string) and those merged
    from 'both' mates."""
    out = {}
    tallies = dict(insertions=0, both=0)
    for rname, cuts, ins1, ins2 in units(remap_text, q_cutoffs):
        for c in cuts:
            for key, string in merge_inserts(ins1, ins2, q_cutoff=c).items():
                k = rname, c, key, string
                out[k] = out.get(k, 0) + 1
                tallies['insertions'] += 1
                tallies['both'] += key in ins1 and key in ins2
    return out, tallies


def ordered(count_dict):
    """conseq_ins.csv's rows of {(refname, qcut, key, string): units}:
    references as Python sorts str, cutoff, position, count descending,
    string as bytes."""
    return [[r, c, p, s, n] for (r, c, p, s), n in
            sorted(count_dict.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], -kv[1],
                                                       kv[0][3].encode()))]


def to_text(rows):
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows(rows)
    return out.getvalue()


def conseq_ins(remap_text, q_cutoffs=(15,)):
    """conseq_ins.csv text of remap.csv text."""
    return to_text(ordered(counts(remap_text, q_cutoffs)[0]))


def totals(conseq_ins_text):
    """{(refname, qcut, pos): count summed over the strings} of the text."""
    out = {}
    for r in csv.DictReader(io.StringIO(conseq_ins_text)):
        k = r['refname'], int(r['qcut']), int(r['pos'])
        out[k] = out.get(k, 0) + int(r['count'])
    return out

"""Hand-written remap.csv texts for sam2aln's mate concordance, with the
counts each must give worked out by hand from the rules (DESIGN.md section 6,
"Mate concordance"): tests/test_concordance_oracle.py holds the oracle to
them, tests/test_gpu_concordance.py the device pass.

A read's default SEQ agrees with the reference it lies on (the base at
position y is 'ACGT'[y % 4]; inserted and clipped bases are 'T'), so two mates
agree wherever both hold a base unless a case edits one of them.  The default
QUAL is 'I' (quality 40)."""
import csv
import io
import re

HEADER = ['qname', 'flag', 'rname', 'pos', 'mapq', 'cigar', 'rnext', 'pnext', 'tlen', 'seq', 'qual']
FWD, REV, UNPAIRED = 99, 147, 0          # read 1 forward, read 2 reversed
FWD1, FWD2 = 67, 131                     # both mates forward


def row(qname, flag, rname, pos, cigar, edit=None, qual='I', quals=None):
    """One remap.csv row.  edit: {read index: byte}; quals: {read index: quality byte}."""
    seq, y = [], pos
    if cigar == '*':
        seq = list('ACGT')
    for n, op in re.findall(r'(\d+)([MIDS])', cigar):
        for _ in range(int(n)):
            if op == 'M':
                seq.append('ACGT'[y % 4])
                y += 1
            elif op == 'D':
                y += 1
            else:
                seq.append('T')
    q = [qual] * len(seq)
    for x, c in (edit or {}).items():
        seq[x] = c
    for x, c in (quals or {}).items():
        q[x] = c
    return [qname, flag, rname, pos, 44, cigar, '=', pos, 0, ''.join(seq), ''.join(q)]


def text(rows):
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows(rows)
    return out.getvalue()


def _positions(ref, lo, hi, **special):
    """overlap 1 at lo..hi of ref; special: name -> positions that also count there."""
    names = ['overlap', 'mismatch', 'indel', 'nocall', 'unresolved']
    out = {(ref, p): [1, 0, 0, 0, 0] for p in range(lo, hi + 1)}
    for name, where in special.items():
        for p in where:
            out[ref, p][names.index(name)] = 1
    return out


def _reads(*mates):
    """mates: (read, cycles compared, {cycle: quality other than 40}, cycles that mismatch)."""
    out = {}
    for read, cycles, quals, bad in mates:
        for c in cycles:
            for key in ((read, 'cycle', c), (read, 'quality', quals.get(c, 40))):
                cell = out.setdefault(key, [0, 0])
                cell[0] += 1
                cell[1] += c in bad
    return out


def _r(lo, hi):
    return range(lo, hi + 1)


def _clean(n, p1, len1, p2, len2, ref='R1', flags=(FWD, REV)):
    """A forward read 1 of len1 M at p1 and a reversed read 2 of len2 M at p2
    that agree everywhere: overlap lo..hi, read 1 at cycles y - p1 + 1, read 2
    at cycles len2 - (y - p2)."""
    lo, hi = max(p1, p2), min(p1 + len1, p2 + len2) - 1
    rows = [row(n, flags[0], ref, p1, '%dM' % len1), row(n, flags[1], ref, p2, '%dM' % len2)]
    if hi < lo:
        return rows, {}, {}
    return (rows, _positions(ref, lo, hi),
            _reads((1, [y - p1 + 1 for y in _r(lo, hi)], {}, ()),
                   (2, [len2 - (y - p2) for y in _r(lo, hi)], {}, ())))


_MANY = '2M1D' * 40 + '2M'       # 81 ops: 82 read bases over 122 positions
_MANY_M = [10 + 3 * k + j for k in range(40) for j in (0, 1)] + [130, 131]

# name -> (rows, {(refname, pos): [overlap, mismatch, indel, nocall, unresolved]},
#          {(read, by, value): [compared, mismatch]})
CASES = {
    # ---- the wave's chunk edges: 10..29 and 29..48 share position 29 alone ----
    'overlap_1': _clean('a', 10, 20, 29, 20),
    'overlap_64': _clean('a', 10, 100, 46, 100),      # 46..109
    'overlap_65': _clean('a', 10, 100, 45, 100),      # 45..109
    'overlap_129': _clean('a', 10, 150, 31, 150),     # 31..159
    # ---- 10..29 and 30..49 touch; 10..29 and 40..59 leave a gap ----
    'touching': _clean('a', 10, 20, 30, 20),
    'gap': _clean('a', 10, 20, 40, 20),
    # read 2 (20..29) inside read 1 (10..59)
    'inside': _clean('a', 10, 50, 20, 10),
    # read 2's row comes first: it is the unit's row 1
    'read2_first': ([row('a', REV, 'R1', 15, '20M'), row('a', FWD, 'R1', 10, '20M')],
                    _positions('R1', 15, 29),
                    _reads((1, _r(6, 20), {}, ()), (2, _r(6, 20), {}, ()))),
    # read 1 deletes 20, 21, which read 2 holds: two indels (' ' against 'I' is
    # 41 apart: resolved).  Read 1's bases are cycles 1..20; read 2 (22 bases,
    # reversed) is compared at indexes 0..9 and 12..21: cycles 22..13, 10..1
    'd_one_mate': ([row('a', FWD, 'R1', 10, '10M2D10M'), row('a', REV, 'R1', 10, '22M')],
                   _positions('R1', 10, 31, indel=(20, 21)),
                   _reads((1, _r(1, 20), {}, ()), (2, list(_r(1, 10)) + list(_r(13, 22)), {}, ()))),
    # both delete 20, 21: '-' equals '-'
    'd_both': ([row('a', FWD, 'R1', 10, '10M2D10M'), row('a', REV, 'R1', 10, '10M2D10M')],
               _positions('R1', 10, 31),
               _reads((1, _r(1, 20), {}, ()), (2, _r(1, 20), {}, ()))),
    # read 1 inserts three bases after its tenth: its cycles 11..13 lie on no
    # position, and the bases after them are cycles 14..23
    'i_in_overlap': ([row('a', FWD, 'R1', 10, '10M3I10M'), row('a', REV, 'R1', 10, '20M')],
                     _positions('R1', 10, 29),
                     _reads((1, list(_r(1, 10)) + list(_r(14, 23)), {}, ()), (2, _r(1, 20), {}, ()))),
    # five clipped bases first: the aligned ones are cycles 6..20
    'lead_s': ([row('a', FWD, 'R1', 10, '5S15M'), row('a', REV, 'R1', 10, '15M')],
               _positions('R1', 10, 24),
               _reads((1, _r(6, 20), {}, ()), (2, _r(1, 15), {}, ()))),
    # the reversed mate has 14 bases, four of them clipped at its 3' end in the
    # row (its 5' end on the sequencer): indexes 0..7 are cycles 14..7
    'reverse_mate': ([row('a', FWD, 'R1', 10, '10M'), row('a', REV, 'R1', 12, '10M4S')],
                     _positions('R1', 12, 19),
                     _reads((1, _r(3, 10), {}, ()), (2, _r(7, 14), {}, ()))),
    # both forward: read 2's indexes 0..7 are cycles 1..8
    'both_forward': ([row('a', FWD1, 'R1', 10, '10M'), row('a', FWD2, 'R1', 12, '10M')],
                     _positions('R1', 12, 19),
                     _reads((1, _r(3, 10), {}, ()), (2, _r(1, 8), {}, ()))),
    # 'N' against a base at 13: nocall, and unresolved since the qualities are
    # equal; neither mate is compared there (read 1 cycle 4, read 2 cycle 7)
    'n_vs_base': ([row('a', FWD, 'R1', 10, '10M', edit={3: 'N'}), row('a', REV, 'R1', 10, '10M')],
                  _positions('R1', 10, 19, nocall=(13,), unresolved=(13,)),
                  _reads((1, [c for c in _r(1, 10) if c != 4], {}, ()),
                         (2, [c for c in _r(1, 10) if c != 7], {}, ()))),
    'n_vs_n': ([row('a', FWD, 'R1', 10, '10M', edit={3: 'N'}),
                row('a', REV, 'R1', 10, '10M', edit={3: 'N'})],
               _positions('R1', 10, 19),
               _reads((1, [c for c in _r(1, 10) if c != 4], {}, ()),
                      (2, [c for c in _r(1, 10) if c != 7], {}, ()))),
    # a mismatch at 13 ('C' on the reference) with qualities 'I' and 'E', 4
    # apart: unresolved; with 'I' and 'D', 5 apart: resolved
    'q_delta_4': ([row('a', FWD, 'R1', 10, '10M', edit={3: 'G'}),
                   row('a', REV, 'R1', 10, '10M', quals={3: 'E'})],
                  _positions('R1', 10, 19, mismatch=(13,), unresolved=(13,)),
                  _reads((1, _r(1, 10), {}, (4,)), (2, _r(1, 10), {7: 36}, (7,)))),
    'q_delta_5': ([row('a', FWD, 'R1', 10, '10M', edit={3: 'G'}),
                   row('a', REV, 'R1', 10, '10M', quals={3: 'D'})],
                  _positions('R1', 10, 19, mismatch=(13,)),
                  _reads((1, _r(1, 10), {}, (4,)), (2, _r(1, 10), {7: 35}, (7,)))),
    # a '-' the read itself holds, under an M op, against the mate's base: an
    # indel by position, a compared and mismatching base by read
    'literal_dash': ([row('a', FWD, 'R1', 10, '10M', edit={3: '-'}), row('a', REV, 'R1', 10, '10M')],
                     _positions('R1', 10, 19, indel=(13,), unresolved=(13,)),
                     _reads((1, _r(1, 10), {}, (4,)), (2, _r(1, 10), {}, (7,)))),
    # 81 CIGAR ops: a deletion after every two bases, against a mate that holds
    # all 122 positions: 40 indels; read 2's index is y - 10, its cycle 122 - that
    'many_ops': ([row('a', FWD, 'R1', 10, _MANY), row('a', REV, 'R1', 10, '122M')],
                 _positions('R1', 10, 131, indel=[12 + 3 * k for k in range(40)]),
                 _reads((1, _r(1, 82), {}, ()), (2, [122 - (y - 10) for y in _MANY_M], {}, ()))),
    # 1 000-base reads that share 501..1000; 2 000-base reads that share 1001..2000
    'read_1000': _clean('a', 1, 1000, 501, 1000),
    'read_2000': _clean('a', 1, 2000, 1001, 2000),
    # two references: zeta first in the file, alpha first in the output
    'two_refs': (_clean('a', 10, 10, 12, 10, ref='zeta')[0] + _clean('b', 5, 4, 5, 4, ref='alpha')[0],
                 {**_positions('alpha', 5, 8), **_positions('zeta', 12, 19)},
                 _reads((1, _r(3, 10), {}, ()), (2, _r(3, 10), {}, ()),
                        (1, _r(1, 4), {}, ()), (2, _r(1, 4), {}, ()))),
    # units that do not reach the merge, and an unpaired one that does
    'unmatched': ([row('a', FWD, 'R1', 10, '10M')], {}, {}),
    'bad_cigar': ([row('a', FWD, 'R1', 10, '10M'), row('a', REV, 'R1', 10, '*')], {}, {}),
    'two_refs_pair': ([row('a', FWD, 'R1', 10, '10M'), row('a', REV, 'R2', 10, '10M')], {}, {}),
    'unpaired': ([row('a', UNPAIRED, 'R1', 10, '10M')], {}, {}),
    # every base below the cutoff: manyNs in failed.csv, counted all the same
    'many_ns': ([row('a', FWD, 'R1', 10, '10M', qual='#'), row('a', REV, 'R1', 10, '10M', qual='#')],
                _positions('R1', 10, 19),
                _reads((1, _r(1, 10), dict.fromkeys(_r(1, 10), 2), ()),
                       (2, _r(1, 10), dict.fromkeys(_r(1, 10), 2), ()))),
}
FAILED_CAUSE = {'unmatched': 'unmatched', 'bad_cigar': 'badCigar', 'two_refs_pair': '2refs',
                'many_ns': 'manyNs'}
NOT_COUNTED = ('unmatched', 'bad_cigar', 'two_refs_pair', 'unpaired', 'touching', 'gap')


def expected_texts(positions, reads):
    """(concordance.csv, cycle_concordance.csv) of a case's expected counts."""
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(['refname', 'pos', 'overlap', 'mismatch', 'indel', 'nocall', 'unresolved'])
    w.writerows([r, p] + positions[r, p] for r, p in sorted(positions))
    out2 = io.StringIO()
    w = csv.writer(out2, lineterminator='\n')
    w.writerow(['read', 'by', 'value', 'compared', 'mismatch'])
    w.writerows(list(k) + reads[k] for k in sorted(reads))
    return out.getvalue(), out2.getvalue()


def combined():
    """Every case in one text (qnames made distinct): the counts add up."""
    rows, positions, reads = [], {}, {}
    for name, (case_rows, want_p, want_r) in CASES.items():
        rows += [[name + '.' + r[0]] + r[1:] for r in case_rows]
        for total, want in ((positions, want_p), (reads, want_r)):
            for key, counts in want.items():
                total[key] = [a + b for a, b in zip(total.get(key, [0] * len(counts)), counts)]
    return rows, positions, reads

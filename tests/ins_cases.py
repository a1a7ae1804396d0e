"""Hand-written remap.csv texts for sam2aln's merged insertions, with the
conseq_ins.csv rows each must give worked out by hand from the rule
("Merged insertions"): tests/test_ins_oracle.py holds
the oracle to them, tests/test_gpu_conseq_ins.py the device pass.

Qualities: 'I' (Q40) passes every cutoff used here; '#' (Q2) fails cutoff 15,
whose character is '0'; digits are Q15 + their distance from '0'."""
import csv
import io

HEADER = ['qname', 'flag', 'rname', 'pos', 'mapq', 'cigar', 'rnext', 'pnext', 'tlen', 'seq', 'qual']
FWD, REV, UNPAIRED = 99, 147, 0


def read(qname, flag, rname, pos, *pieces):
    """One remap.csv row from CIGAR pieces: 'S3', 'M5', 'D2' (quality 'I';
    the base aligned to consensus position x is 'ACGT'[x % 4], so mates agree
    where they overlap), ('I', seq) or ('I', seq, qual) for an insertion, ('M',
    n, qual char) for aligned bases of another quality, or a literal CIGAR
    op without bases such as '0I'."""
    cigar, seq, qual, ref = '', '', '', pos

    def aligned(n):
        return ''.join('ACGT'[(ref + k) % 4] for k in range(n))
    for p in pieces:
        if isinstance(p, tuple) and p[0] == 'I':
            s = p[1]
            q = p[2] if len(p) > 2 else 'I' * len(s)
            assert len(s) == len(q)
            cigar += '%dI' % len(s)
            seq += s
            qual += q
        elif isinstance(p, tuple):
            cigar += '%d%s' % (p[1], p[0])
            seq += aligned(p[1])
            qual += p[2] * p[1]
            ref += p[1]
        elif p[0].isdigit():
            cigar += p
        else:
            n = int(p[1:])
            cigar += '%d%s' % (n, p[0])
            if p[0] != 'D':
                seq += aligned(n)
                qual += 'I' * n
            if p[0] != 'S':
                ref += n
    return [qname, flag, rname, pos, 44, cigar, '=', pos, 0, seq, qual]


def text(rows):
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows(rows)
    return out.getvalue()


def expected_text(rows):
    """conseq_ins.csv of rows [refname, qcut, pos, insert, count], in order."""
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(['refname', 'qcut', 'pos', 'insert', 'count'])
    w.writerows(rows)
    return out.getvalue()


def _pair(name, rname, pos1, pieces1, pos2, pieces2):
    return [read(name, FWD, rname, pos1, *pieces1), read(name, REV, rname, pos2, *pieces2)]


def _same_key(ins1, ins2):
    """A pair whose mates both insert after consensus position 13."""
    return _pair('p', 'R1', 10, ['M4', ('I',) + ins1, 'M6'], 10, ['M4', ('I',) + ins2, 'M6'])


# name -> (rows, q-cutoffs, [[refname, qcut, pos, insert, count]] in file order)
CASES = {
    # ---- keying ----
    # POS 10, 3S4M: the insertion follows consensus position 9 + 4 = 13
    # (insert.csv's pos counts the clip: 9 + 7 = 16)
    'after_soft_clip': ([read('a', UNPAIRED, 'R1', 10, 'S3', 'M4', ('I', 'GG'), 'M4')], [15],
                        [['R1', 15, 13, 'GG', 1]]),
    # 4M2D: 9 + 6 = 15 (insert.csv's pos leaves the deletion out: 13)
    'after_deletion': ([read('a', UNPAIRED, 'R1', 10, 'M4', 'D2', ('I', 'TTT'), 'M4')], [15],
                       [['R1', 15, 15, 'TTT', 1]]),
    # POS 5: 4 + 3 = 7, then 4 + 6 = 10 (the first insertion is not counted in)
    'two_in_one_read': ([read('a', UNPAIRED, 'R1', 5, 'M3', ('I', 'A'), 'M3', ('I', 'CC'), 'M3')], [15],
                        [['R1', 15, 7, 'A', 1], ['R1', 15, 10, 'CC', 1]]),
    # 2I1I share key 7: the later one stands, also across an S op and a 0D
    'adjacent_later_wins': ([read('a', UNPAIRED, 'R1', 5, 'M3', ('I', 'AA'), ('I', 'C'), 'M3'),
                             read('b', UNPAIRED, 'R1', 5, 'M3', ('I', 'TT'), 'S1', '0D', ('I', 'G'), 'M3')],
                            [15], [['R1', 15, 7, 'C', 1], ['R1', 15, 7, 'G', 1]]),
    # 0I records nothing, and replaces nothing
    'zero_length': ([read('a', UNPAIRED, 'R1', 5, 'M3', '0I', 'M3'),
                     read('b', UNPAIRED, 'R1', 5, 'M3', ('I', 'GG'), '0I', 'M3')], [15],
                    [['R1', 15, 7, 'GG', 1]]),
    # before the first M at POS 1: key 0
    'before_first_base': ([read('a', UNPAIRED, 'R1', 1, ('I', 'GT'), 'M5')], [15],
                          [['R1', 15, 0, 'GT', 1]]),
    # mate 1 inserts after 13, mate 2 (POS 12, 5M) after 11 + 5 = 16
    'mates_different_keys': (_pair('p', 'R1', 10, ['M4', ('I', 'A'), 'M6'], 12, ['M5', ('I', 'CC'), 'M4']),
                             [15], [['R1', 15, 13, 'A', 1], ['R1', 15, 16, 'CC', 1]]),
    # ---- one key, both mates ----
    'both_agree': (_same_key(('ACG',), ('ACG',)), [15], [['R1', 15, 13, 'ACG', 1]]),
    # A(I) / C(5): mate 1 higher by 20, A.  C(5) / G(I): mate 2 higher, G.
    # G(7) / T(9): 2 apart, N.  T / T: T.
    'both_disagree': (_same_key(('ACGT', 'I57I'), ('CGTT', '5I9I')), [15], [['R1', 15, 13, 'AGNT', 1]]),
    # mate 1 fails (min '#'), mate 2 passes (min '2'): merged with mate 1's
    # raw string -- A(I) / G(2) gives mate 1's A, C(#) / C(2) gives C
    'mate1_fails_mate2_passes': (_same_key(('AC', 'I#'), ('GC', '22')), [15], [['R1', 15, 13, 'AC', 1]]),
    # mate 2 fails: mate 1's string alone
    'mate1_passes_mate2_fails': (_same_key(('AC',), ('GG', 'I#')), [15], [['R1', 15, 13, 'AC', 1]]),
    'both_fail': (_same_key(('AC', 'I#'), ('AC', '#I')), [15], []),
    # mate 1 is the longer one: it becomes seq2 and the tail past mate 2's
    # two bases is judged by mate 1's qualities -- G(I), T(I), A(#) -> N
    'longer_mate1': (_same_key(('ACGTA', 'IIII#'), ('AC',)), [15], [['R1', 15, 13, 'ACGTN', 1]]),
    # mate 2 the longer one, mate 1 passing: T(I) / A(I) differ by 0 -> N
    'longer_mate2': (_same_key(('AT',), ('AAG',)), [15], [['R1', 15, 13, 'ANG', 1]]),
    # ---- units ----
    'unpaired': ([read('a', UNPAIRED, 'R1', 20, 'M5', ('I', 'CAT'), 'M5')], [15],
                 [['R1', 15, 24, 'CAT', 1]]),
    # every base Q10 ('+'): all N at cutoff 15 (manyNs), none at cutoff 0,
    # where the insertion's qualities pass too
    'many_ns_at_15': (_pair('p', 'R1', 10, [('M', 4, '+'), ('I', 'GA', '++'), ('M', 6, '+')],
                            10, [('M', 4, '+'), ('I', 'GA', '++'), ('M', 6, '+')]), [0, 15],
                      [['R1', 0, 13, 'GA', 1]]),
    # unmatched (a paired flag and no mate), badCigar ('*'), 2refs: not counted
    'unmatched': ([read('a', FWD, 'R1', 10, 'M4', ('I', 'GG'), 'M4')], [15], []),
    'bad_cigar': ([read('a', FWD, 'R1', 10, 'M4', ('I', 'GG'), 'M4'),
                   ['a', REV, 'R1', 10, 44, '*', '=', 10, 0, 'ACGT', 'IIII']], [15], []),
    'two_refs_pair': ([read('a', FWD, 'R1', 10, 'M4', ('I', 'GG'), 'M4'),
                       read('a', REV, 'R2', 10, 'M4', ('I', 'GG'), 'M4')], [15], []),
    # references in file order zeta, 'b,1' (quoted), alpha: sorted as str
    'two_refs': ([read('a', UNPAIRED, 'zeta', 10, 'M4', ('I', 'G'), 'M4'),
                  read('b', UNPAIRED, 'b,1', 7, 'M4', ('I', 'TT'), 'M4'),
                  read('c', UNPAIRED, 'alpha', 50, 'M2', ('I', 'C'), 'M5')], [15],
                 [['alpha', 15, 51, 'C', 1], ['b,1', 15, 10, 'TT', 1], ['zeta', 15, 13, 'G', 1]]),
    # one key: TT twice comes first, then CC and GG, once each, by string;
    # position 9 before position 13 whatever the counts
    'count_then_string': ([read('a', UNPAIRED, 'R1', 10, 'M4', ('I', 'GG'), 'M4'),
                           read('b', UNPAIRED, 'R1', 10, 'M4', ('I', 'TT'), 'M4'),
                           read('c', UNPAIRED, 'R1', 10, 'M4', ('I', 'CC'), 'M4'),
                           read('d', UNPAIRED, 'R1', 10, 'M4', ('I', 'TT'), 'M4'),
                           read('e', UNPAIRED, 'R1', 6, 'M4', ('I', 'A'), 'M8')], [15],
                          [['R1', 15, 9, 'A', 1], ['R1', 15, 13, 'TT', 2], ['R1', 15, 13, 'CC', 1],
                           ['R1', 15, 13, 'GG', 1]]),
}
FAILED_CAUSE = {'unmatched': 'unmatched', 'bad_cigar': 'badCigar', 'two_refs_pair': '2refs'}


def combined():
    """Every case in one text at cutoff 15 (qnames made distinct): the counts
    of equal rows add up; many_ns_at_15 gives nothing at this cutoff."""
    rows, counts = [], {}
    for name, (case_rows, _, want) in CASES.items():
        rows += [[name + '.' + r[0]] + r[1:] for r in case_rows]
        for rname, qcut, pos, ins, n in want:
            if qcut == 15:
                counts[rname, pos, ins] = counts.get((rname, pos, ins), 0) + n
    ordered = sorted(counts.items(), key=lambda kv: (kv[0][0], kv[0][1], -kv[1], kv[0][2].encode()))
    return rows, [[r, 15, p, s, n] for (r, p, s), n in ordered]

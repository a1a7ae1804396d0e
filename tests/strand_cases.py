"""Hand-written remap.csv texts for sam2aln's strand support, with the counts
each must give worked out by hand from the rules ("Strand
support"), not from the oracle: tests/test_strand_oracle.py holds the oracle
to them, tests/test_gpu_strand.py the device pass.

Rows come from concordance_cases.row: a read's default SEQ agrees with the
reference it lies on (the base at position y is 'ACGT'[y % 4]; inserted and
clipped bases are 'T') and its default QUAL is 'I' (quality 40, byte 73).  The
cutoff 15 is the byte '0' (48); a D op's quality is ' ' (32), padding's '!'."""
import csv
import io

from concordance_cases import FWD, FWD1, FWD2, REV, UNPAIRED, row, text  # noqa: F401 (re-exported)

REV1, REV2 = 83, 147                     # both mates reversed
UNPAIRED_REV = 16
BASES = 'ACGT-'
HEADER = ['refname', 'qcut', 'pos'] + [n + s for n in ('A', 'C', 'G', 'T', 'del')
                                       for s in ('_fwd', '_rev', '_both')]


def _r(lo, hi):
    return range(lo, hi + 1)


def _want(*parts, ref='R1', q=15):
    """parts: (positions, 'fwd' | 'rev' | 'both'[, base]); the base defaults to
    the reference's, 'ACGT'[y % 4]."""
    out = {}
    for positions, how, *base in parts:
        for y in positions:
            k = 3 * BASES.index(base[0] if base else 'ACGT'[y % 4])
            v = out.setdefault((ref, q, y), [0] * 15)
            v[k] += how in ('fwd', 'both')
            v[k + 1] += how in ('rev', 'both')
            v[k + 2] += how == 'both'
    return out


def _pair(edit1=None, quals1=None, edit2=None, quals2=None):
    """Read 1 forward and read 2 reversed, both 10M at 10: position 13 ('C') is index 3."""
    return [row('a', FWD, 'R1', 10, '10M', edit=edit1, quals=quals1),
            row('a', REV, 'R1', 10, '10M', edit=edit2, quals=quals2)]


_REST = [y for y in _r(10, 19) if y != 13]

# name -> (rows, cutoffs, {(refname, qcut, pos): [15 counts in HEADER's order]})
CASES = {
    # ---- 10..29 forward, 20..39 reversed ----
    'fwd_rev': ([row('a', FWD, 'R1', 10, '20M'), row('a', REV, 'R1', 20, '20M')], [15],
                _want((_r(10, 19), 'fwd'), (_r(20, 29), 'both'), (_r(30, 39), 'rev'))),
    # read 2's row comes first: it is the unit's row 1 and the longer padded read
    'read2_first': ([row('a', REV, 'R1', 15, '20M'), row('a', FWD, 'R1', 10, '20M')], [15],
                    _want((_r(10, 14), 'fwd'), (_r(15, 29), 'both'), (_r(30, 34), 'rev'))),
    # same-strand pairs: two supporting mates on one strand add 1, not 2
    'both_forward': ([row('a', FWD1, 'R1', 10, '10M'), row('a', FWD2, 'R1', 12, '10M')], [15],
                     _want((_r(10, 21), 'fwd'))),
    'both_reversed': ([row('a', REV1, 'R1', 10, '10M'), row('a', REV2, 'R1', 12, '10M')], [15],
                      _want((_r(10, 21), 'rev'))),
    # an unpaired read is not masked: quality '!' still counts
    'unpaired_fwd': ([row('a', UNPAIRED, 'R1', 10, '10M')], [15], _want((_r(10, 19), 'fwd'))),
    'unpaired_rev': ([row('a', UNPAIRED_REV, 'R1', 10, '10M', qual='!')], [15], _want((_r(10, 19), 'rev'))),
    'unpaired_n': ([row('a', UNPAIRED, 'R1', 10, '10M', edit={3: 'N'})], [15], _want((_REST, 'fwd'))),
    # ---- the mates disagree at 13: 'G' (read 1) against 'C' ----
    # 'I' against 'D', 5 apart: read 1 wins, its strand alone
    'resolved': (_pair(edit1={3: 'G'}, quals2={3: 'D'}), [15],
                 _want((_REST, 'both'), ([13], 'fwd', 'G'))),
    # 'I' against 'E', 4 apart: 'N'
    'unresolved': (_pair(edit1={3: 'G'}, quals2={3: 'E'}), [15], _want((_REST, 'both'))),
    # '0' against '#', 13 apart, but the winner is not above the cutoff: 'N'
    'winner_at_cutoff': (_pair(edit1={3: 'G'}, quals1={3: '0'}, quals2={3: '#'}), [15],
                         _want((_REST, 'both'))),
    # ---- the mates agree at 13 ----
    # one quality below the cutoff: the base stands, and both mates support it
    'agree_one_low': (_pair(quals1={3: '#'}), [15], _want((_r(10, 19), 'both'))),
    'agree_both_low': (_pair(quals1={3: '#'}, quals2={3: '#'}), [15], _want((_REST, 'both'))),
    # ---- deletions ----
    'd_both': ([row('a', FWD, 'R1', 10, '10M2D10M'), row('a', REV, 'R1', 10, '10M2D10M')], [15],
               _want((list(_r(10, 19)) + list(_r(22, 31)), 'both'), ([20, 21], 'both', '-'))),
    # read 2 (10..21, deleting 15 and 16) is the shorter padded read; read 1
    # starts at 30.  At 15, 16 both hold '-', read 1's being padding: read 2
    # alone supports.  22..29 lie in the gap between the mates: 'n'
    'd_one_padding': ([row('a', FWD, 'R1', 30, '10M'), row('a', REV, 'R1', 10, '5M2D5M')], [15],
                      _want((list(_r(10, 14)) + list(_r(17, 21)), 'rev'), ([15, 16], 'rev', '-'),
                            (_r(30, 39), 'fwd'))),
    # read 1 deletes 20, 21 (quality ' '), read 2 holds bases there: quality 37
    # ('F') wins for read 2's strand; quality 2 ('#', 3 apart) gives 'N'
    'd_vs_base_37': ([row('a', FWD, 'R1', 10, '10M2D10M'),
                      row('a', REV, 'R1', 10, '22M', quals={10: 'F', 11: 'F'})], [15],
                     _want((list(_r(10, 19)) + list(_r(22, 31)), 'both'), ([20, 21], 'rev'))),
    'd_vs_base_2': ([row('a', FWD, 'R1', 10, '10M2D10M'),
                     row('a', REV, 'R1', 10, '22M', quals={10: '#', 11: '#'})], [15],
                    _want((list(_r(10, 19)) + list(_r(22, 31)), 'both'))),
    # the byte '%' (37) is 5 above ' ': the base wins at cutoff 0 ('!'), not at 15
    'd_vs_base_byte_37': ([row('a', FWD, 'R1', 10, '10M2D10M'),
                           row('a', REV, 'R1', 10, '22M', quals={10: '%', 11: '%'})], [0, 15],
                          {**_want((list(_r(10, 19)) + list(_r(22, 31)), 'both'), ([20, 21], 'rev'), q=0),
                           **_want((list(_r(10, 19)) + list(_r(22, 31)), 'both'))}),
    # ---- I and S ops consume read only: 5S5M3I5M lies on 10..19 ----
    'i_and_s': ([row('a', FWD, 'R1', 10, '5S5M3I5M'), row('a', REV, 'R1', 10, '10M4S')], [15],
                _want((_r(10, 19), 'both'))),
    # ---- 'N' in a read ----
    # equal qualities: 'N'; read 1's 'N' at quality 2: read 2's base wins
    'n_tie': (_pair(edit1={3: 'N'}), [15], _want((_REST, 'both'))),
    'n_low': (_pair(edit1={3: 'N'}, quals1={3: '#'}), [15], _want((_REST, 'both'), ([13], 'rev'))),
    # ---- units that do not count ----
    'unmatched': ([row('a', FWD, 'R1', 10, '10M')], [15], {}),
    'bad_cigar': ([row('a', FWD, 'R1', 10, '10M'), row('a', REV, 'R1', 10, '*')], [15], {}),
    'two_refs_pair': ([row('a', FWD, 'R1', 10, '10M'), row('a', REV, 'R2', 10, '10M')], [15], {}),
    'many_ns': ([row('a', FWD, 'R1', 10, '10M', qual='#'), row('a', REV, 'R1', 10, '10M', qual='#')], [15], {}),
    # quality 20 ('5') everywhere: every base at cutoff 10, manyNs at 30
    'many_ns_at_30': ([row('a', FWD, 'R1', 10, '10M', qual='5'), row('a', REV, 'R1', 10, '10M', qual='5')],
                      [10, 30], _want((_r(10, 19), 'both'), q=10)),
    # cutoffs given unsorted: 30's rows first; 13 is 'N' at 30 only
    'unsorted_cutoffs': (_pair(quals1={3: '5'}, quals2={3: '5'}), [30, 10],
                         {**_want((_REST, 'both'), q=30), **_want((_r(10, 19), 'both'), q=10)}),
    # zeta first in the file, alpha first in the output
    'two_refs': ([row('a', FWD, 'zeta', 10, '10M'), row('a', REV, 'zeta', 12, '10M'),
                  row('b', FWD, 'alpha', 5, '4M'), row('b', REV, 'alpha', 5, '4M')], [15],
                 {**_want((_r(10, 11), 'fwd'), (_r(12, 19), 'both'), (_r(20, 21), 'rev'), ref='zeta'),
                  **_want((_r(5, 8), 'both'), ref='alpha')}),
    # ---- merged lengths of 64, 65 and 129: the wave's step edges ----
    'merged_64': ([row('a', FWD, 'R1', 1, '40M'), row('a', REV, 'R1', 25, '40M')], [15],
                  _want((_r(1, 24), 'fwd'), (_r(25, 40), 'both'), (_r(41, 64), 'rev'))),
    'merged_65': ([row('a', FWD, 'R1', 1, '40M'), row('a', REV, 'R1', 26, '40M')], [15],
                  _want((_r(1, 25), 'fwd'), (_r(26, 40), 'both'), (_r(41, 65), 'rev'))),
    'merged_129': ([row('a', FWD, 'R1', 1, '100M'), row('a', REV, 'R1', 30, '100M')], [15],
                   _want((_r(1, 29), 'fwd'), (_r(30, 100), 'both'), (_r(101, 129), 'rev'))),
    # ---- the forward read never starts: read 1 (4S6D at 3) expands to six
    # '-' over 3..8, eight padded bytes in all, read 2 holds 10..19.  merge_pairs
    # drops the indexes below 8: mseq = 'n' + read 2's ten bases, mseq[j] the
    # base of position j + 9.  Support is looked up at y = j + 1 all the same:
    # read 2 holds 10 ('G') and 11 ('T'), and mseq[9], mseq[10] are the bases of
    # 18 and 19, 'G' and 'T' again.  Nothing else matches ----
    'forward_never_starts': ([row('a', FWD, 'R1', 3, '4S6D'), row('a', REV, 'R1', 10, '10M')], [15],
                             _want(([10, 11], 'rev'))),
}
FAILED_CAUSE = {'unmatched': 'unmatched', 'bad_cigar': 'badCigar', 'two_refs_pair': '2refs',
                'many_ns': 'manyNs', 'many_ns_at_30': 'manyNs'}
HEADER_ALONE = ('unmatched', 'bad_cigar', 'two_refs_pair', 'many_ns')


def expected_text(want, cuts):
    """strand.csv of a case's expected counts."""
    out = io.StringIO()
    w = csv.writer(out, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows([name, q, pos] + want[name, q, pos]
                for name, q, pos in sorted(want, key=lambda k: (k[0], cuts.index(k[1]), k[2])))
    return out.getvalue()


def combined(cuts=(15,)):
    """Every case that runs at `cuts` in one text (qnames made distinct): the counts add up."""
    rows, total = [], {}
    for name, (case_rows, case_cuts, want) in CASES.items():
        if list(case_cuts) != list(cuts):
            continue
        rows += [[name + '.' + r[0]] + r[1:] for r in case_rows]
        for key, counts in want.items():
            total[key] = [a + b for a, b in zip(total.get(key, [0] * 15), counts)]
    return rows, total

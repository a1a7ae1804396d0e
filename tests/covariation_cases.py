"""Hand-worked rows for the pairwise covariation (DESIGN.md section 6,
"Covariation").  Every expectation below was written out by hand from the
padded text '-' * (frame + offset) + seq cut into codons;
tests/test_covariation_oracle.py holds tests/covariation_oracle.py to them and
tests/test_gpu_covariation.py the device (mh_a2c_gram).

A column mask has bit k set for the character with code k of
'\\0ACDEFGHIKLMNPQRSTVWY*X?-': A 1, E 4, F 5, K 9, N 12, '*' 21, X 22, '?' 23,
'-' 24.  CALLED is the 21 letters and '-'.
"""
CALLED = sum(1 << k for k in range(1, 22)) | 1 << 24


def bit(ch):
    return 1 << '\0ACDEFGHIKLMNPQRSTVWY*X?-'.index(ch)


# name -> (rows [(offset, seq, count)], cols [(frame, codon, mask)], gram)
GRAM = {
    # AAA = K, AGA = R, TTT = F.  K at codon 0: rows 1 and 3 (5 + 2).  F at
    # codon 1, and called at codon 1: rows 1 and 2 (5 + 3); row 3 ends before it.
    'two_positions': (
        [(0, 'AAATTT', 5), (0, 'AGATTT', 3), (0, 'AAA', 2)],
        [(0, 0, bit('K')), (0, 1, bit('F')), (0, 1, CALLED)],
        [[7, 5, 5], [5, 8, 8], [5, 8, 8]]),
    # linkage's 'every_class' rows.  Characters per codon 0..3:
    #   row 1 (2): * - X ?     row 2 (1): * blank T ?     row 3 (3): * ? T Y
    # columns: '*' at 0 {1,2,3}; '-' at 1 {1}; '?' at 1 {3}; X at 2 {1};
    # called at 2 {2,3} (X is not called); called at 1 {1} ('?' is not called)
    'every_class': (
        [(0, 'TAA---ANAA', 2), (0, 'TAAnnnACGT', 1), (0, 'TAAnAnACGTAC', 3)],
        [(0, 0, bit('*')), (0, 1, bit('-')), (0, 1, bit('?')), (0, 2, bit('X')), (0, 2, CALLED), (0, 1, CALLED)],
        [[6, 2, 3, 2, 4, 2],
         [2, 2, 0, 2, 0, 2],
         [3, 0, 3, 0, 3, 0],
         [2, 2, 0, 2, 0, 2],
         [4, 0, 3, 0, 4, 0],
         [2, 2, 0, 2, 0, 2]]),
    # One row at offset 2 in all three frames (linkage's 'three_frames'):
    #   frame 0: --G AAA TTT      ? K F
    #   frame 1: --- GAA ATT T--  blank E I ?
    #   frame 2: --- -GA AAT TT-  blank ? N ?
    'three_frames': (
        [(2, 'GAAATTT', 1)],
        [(1, 1, bit('E')), (2, 2, bit('N')), (0, 1, bit('K')), (1, 0, CALLED), (0, 0, bit('?'))],
        [[1, 1, 1, 0, 1], [1, 1, 1, 0, 1], [1, 1, 1, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 0, 1]]),
    # the same column twice, and a mask of two characters (K or R)
    'equal_columns': (
        [(0, 'AAA', 4), (0, 'AGA', 2), (0, 'GGG', 1)],
        [(0, 0, bit('K')), (0, 0, bit('K')), (0, 0, bit('K') | bit('R'))],
        [[4, 4, 4], [4, 4, 4], [4, 4, 6]]),
}

# name -> (tallies {(region, position): {character: count}}, min_fraction,
#          min_count, max_variants, kept [(region, position, character)], dropped)
SELECT = {
    # RT 10: 100 called, K major; R 8 passes, N 2 is below min_count.  RT 12: A
    # and T tie, the earlier character (A) is the major, T the variant.  PR 5:
    # '-' (del) is a called character like the letters.
    'thresholds_and_the_tie_for_major': (
        {('RT', 10): {'K': 90, 'R': 8, 'N': 2}, ('RT', 12): {'A': 50, 'T': 50}, ('PR', 5): {'L': 95, '-': 5}},
        0.04, 5, 256, [('PR', 5, '-'), ('RT', 10, 'R'), ('RT', 12, 'T')], 0),
    # 3 of 100 is below 0.04
    'fraction': (
        {('RT', 10): {'K': 97, 'R': 3}}, 0.04, 1, 256, [], 0),
    # the cap keeps the largest tallies (T 50, R 8), in pair order
    'the_cap': (
        {('RT', 10): {'K': 90, 'R': 8, 'N': 2}, ('RT', 12): {'A': 50, 'T': 50}, ('PR', 5): {'L': 95, '-': 5}},
        0.04, 5, 2, [('RT', 10, 'R'), ('RT', 12, 'T')], 1),
    # four variants of tally 3: the cap's tie goes by (region, position, character)
    'the_cap_on_a_tie': (
        {('RT', 1): {'A': 10, 'C': 3}, ('PR', 1): {'A': 10, 'C': 3}, ('PR', 2): {'A': 10, 'D': 3, 'C': 3}},
        0.01, 1, 2, [('PR', 1, 'C'), ('PR', 2, 'C')], 2),
}

# Frame 0, RT 1 -> codon 0, RT 2 -> codon 1.  Characters at codons 0 and 1:
#   row 1 (4): K F    row 2 (3): R F    row 3 (2): R W    row 4 (1): K -
#   row 5 (5): K X (NTT: not called at codon 1)    row 6 (6): blank W
# Called at both: rows 1-4, n = 10.  R: rows 2, 3 = 5.  W: row 3 = 2.  '-': row 4 = 1.
#   R / W: n.ab = 2; 10 * 2 > 5 * 2: '+'; r2 = (20 - 10)^2 / (5 * 5 * 2 * 8) = 0.25
#   R / -: n.ab = 0; '-'; r2 = (0 - 5)^2 / (5 * 5 * 1 * 9) = 0.1111
#   W / -: the same codon, no pair
PAIR_ROWS = [(0, 'AAATTTGGG', 4), (0, 'AGATTCGGG', 3), (0, 'AGATGGGGG', 2), (0, 'AAA---GGG', 1),
             (0, 'AAANTTGGG', 5), (3, 'TGGGGG', 6)]
PAIR_VARIANTS = [('RT', 1, 'R'), ('RT', 2, 'W'), ('RT', 2, '-')]
PAIR_PLACE = {('RT', 1): (0, 0), ('RT', 2): (0, 1)}
PAIR_RECORDS = [('RT', 1, 'R', 'RT', 2, 'W', 10, 5, 2, 2), ('RT', 1, 'R', 'RT', 2, '-', 10, 5, 1, 0)]
PAIR_LINES = [['s', '15', 'RT', '1', 'R', 'RT', '2', 'W', '10', '5', '2', '2', '+', '0.2500'],
              ['s', '15', 'RT', '1', 'R', 'RT', '2', '-', '10', '5', '1', '0', '-', '0.1111']]

# (n, n.a, n.b, n.ab) -> (direction, r2)
MEASURES = {
    (46, 13, 19, 13): ('+', '%.4f' % ((46 * 13 - 13 * 19) ** 2 / (13 * 33 * 19 * 27))),
    (4, 2, 2, 1): ('0', '0.0000'),
    (5, 5, 2, 2): ('0', ''),            # a is on every row: no variance
    (9, 3, 0, 0): ('0', ''),
    (10, 5, 5, 0): ('-', '1.0000'),
    (10, 5, 5, 5): ('+', '1.0000'),
}

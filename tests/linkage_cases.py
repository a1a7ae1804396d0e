"""Hand-worked rows for the linked amino acids ("Linked
amino acids"): name -> (rows, sets, min_count, entries, coverage).

rows      [(offset, seq, count)] of one aligned.csv group
sets      [(reading frame, [consensus codons])], placed already
entries   [(set index, count, haplotype bytes)] in report order: sets as
          given, count descending, haplotype bytes ascending
coverage  per set, the rows of haplotypes below min_count included

Every expectation below was written out by hand from the padded text
'-' * (frame + offset) + seq cut into codons; tests/test_linkage_oracle.py
holds tests/linkage_oracle.py to them and tests/test_gpu_linkage.py the
device (mh_a2c_link).
"""

CASES = {
    # codon 0 and codon 2 of frame 0.  AAA = K, AGA = R, TTT = TTC = F.
    # Row 4 starts at codon 1 and row 5 ends before codon 2: blank there.
    'two_linked_positions': (
        [(0, 'AAAGGGTTT', 5), (0, 'AAACCCTTC', 2), (0, 'AGAGGGTTT', 3), (3, 'GGGTTT', 4), (0, 'AAAGGG', 1)],
        [(0, [0, 2])], 1,
        [(0, 7, b'KF'), (0, 3, b'RF')], [10]),
    # TAA = *, three '-' of the row = del, ANA = X, 'A' + padding = partial
    # ('AC' + padding would be T: every ACx is threonine).
    # Second row: 'nnn' is blank, the row does not count.  Third row: 'nAn'
    # is partial, ACG = T, TAC = Y.
    'every_class': (
        [(0, 'TAA---ANAA', 2), (0, 'TAAnnnACGT', 1), (0, 'TAAnAnACGTAC', 3)],
        [(0, [0, 1, 2, 3])], 1,
        [(0, 3, b'*?TY'), (0, 2, b'*-X?')], [5]),
    # One row at offset 2 in all three frames.
    #   frame 0: --G AAA TTT          ? K F
    #   frame 1: --- GAA ATT T--      blank E I ?
    #   frame 2: --- -GA AAT TT-      blank ? N ?
    'three_frames': (
        [(2, 'GAAATTT', 1)],
        [(1, [1, 2]), (1, [0, 1]), (1, [2, 3]), (2, [1, 2, 3]), (0, [0, 1, 2])], 1,
        [(0, 1, b'EI'), (2, 1, b'I?'), (3, 1, b'?N?'), (4, 1, b'?KF')], [1, 0, 1, 1, 1]),
    # K = 2 + 1, F = 2, G = 2, P = 1: the tie goes by the byte, P is cut but covered.
    'ties_and_the_cut': (
        [(0, 'AAA', 2), (0, 'GGG', 2), (0, 'CCC', 1), (0, 'AAG', 1), (0, 'TTT', 2)],
        [(0, [0])], 2,
        [(0, 3, b'K'), (0, 2, b'F'), (0, 2, b'G')], [8]),
    # all at count 1: '*' < '-' < '?' < 'W' < 'X' < 'Y' as bytes
    'byte_order_of_the_characters': (
        [(0, 'TAT', 1), (0, 'ANA', 1), (0, 'TGG', 1), (0, 'A--', 1), (0, '---', 1), (0, 'TAA', 1)],
        [(0, [0])], 1,
        [(0, 1, b'*'), (0, 1, b'-'), (0, 1, b'?'), (0, 1, b'W'), (0, 1, b'X'), (0, 1, b'Y')], [6]),
    # the same string 'K' in two sets stays two entries
    'equal_strings_of_two_sets': (
        [(0, 'AAAAAA', 3), (0, 'AAA', 2)],
        [(0, [0]), (0, [1])], 1,
        [(0, 5, b'K'), (1, 3, b'K')], [5, 3]),
    # the gap between the mates: codons 1 and 2 are 'nnn'.  The pair links
    # codons 0 and 3, but counts for no set that holds codon 1.
    'gap_between_the_mates': (
        [(0, 'AAAnnnnnnTTT', 4)],
        [(0, [0, 3]), (0, [0, 1, 3])], 1,
        [(0, 4, b'KF')], [4, 0]),
}

"""Hand-written aligned.csv rows for the codon classes of amino_detail.csv, with
the [X, partial, del] counts of every codon of every reading frame worked out
by hand from the rule (tests/amino_detail_oracle.py): tests/
test_amino_detail_oracle.py holds the oracle to them, tests/
test_gpu_amino_detail.py the device pass.  The comments spell the padded
codons of each frame and say which '-' are the row's own."""

Z = [0, 0, 0]


def P(n):
    return [0, n, 0]


# name -> ([(offset, seq, count)], {frame: [[X, partial, del] of codons 0 .. ncod - 1]})
CASES = {
    # frame 0: ACG | --- (the row's own: del) | TTT
    # frame 1: -AC | G-- | -TT | T--   (-AC is T/P/..., -TT is I/L/F/V: ambiguous)
    # frame 2: --A | CG- (R whatever follows: a letter) | --T | TT- (F or L)
    'deletion': ([(0, 'ACG---TTT', 5)],
                 {0: [Z, [0, 0, 5], Z], 1: [P(5)] * 4, 2: [P(5), Z, P(5), P(5)]}),
    # offset 1: frame 0 -A- ; frame 1 --A ; frame 2 --- (padding: blank) | A--
    'pad1': ([(1, 'A', 1)], {0: [P(1)], 1: [P(1)], 2: [Z, P(1)]}),
    # offset 2: frame 0 --A | C-- ; frame 1 --- (blank) | AC- (T: a letter) ;
    # frame 2 --- (blank) | -AC
    'pad2': ([(2, 'AC', 2)], {0: [P(2), P(2)], 1: [Z, Z], 2: [Z, P(2)]}),
    # offset 4, codons from 1: frame 0 -AC | G-- ; frame 1 --A | CG- (R) ;
    # frame 2 --- (blank) | ACG
    'pad4': ([(4, 'ACG', 3)], {0: [Z, P(3), P(3)], 1: [Z, P(3), Z], 2: [Z, Z, Z]}),
    # offset 5, codons from 1: frame 0 --A | CGT ; frame 1 --- (blank) | ACG | T-- ;
    # frame 2 --- (blank) | -AC | GT- (V)
    'pad5': ([(5, 'ACGT', 4)], {0: [Z, P(4), Z], 1: [Z, Z, Z, P(4)], 2: [Z, Z, P(4), Z]}),
    # frame 0: --- (own: del) | ACG ; frame 1: --- (1 padding + 2 own: blank) | -AC | G-- ;
    # frame 2: --- (blank) | --A | CG-
    'del_at_start': ([(0, '---ACG', 2)], {0: [[0, 0, 2], Z], 1: [Z, P(2), P(2)], 2: [Z, P(2), Z]}),
    # frame 0: ACG | --- (own: del) ; frame 1: -AC | G-- | --- (1 own + 2 padding: blank) ;
    # frame 2: --A | CG- | --- (blank)
    'del_at_end': ([(0, 'ACG---', 2)], {0: [Z, [0, 0, 2]], 1: [P(2), P(2), Z], 2: [P(2), Z, Z]}),
    # frame 0: ACG | nnn (no base: blank) | ACG ; frame 1: -AC | Gnn | nAC | G-- ;
    # frame 2: --A | CGn (R) | nnA | CG- (R)
    'mate_gap': ([(0, 'ACGnnnACG', 3)], {0: [Z, Z, Z], 1: [P(3)] * 4, 2: [P(3), Z, P(3), Z]}),
    # frame 0: ACn (T) | nnn (blank) | CG- (R) ; frame 1: -AC | nnn (blank) | nCG (T/P/A/S) ;
    # frame 2: --A | Cnn | nnC | G--
    'mate_gap_odd': ([(0, 'ACnnnnCG', 3)], {0: [Z, Z, Z], 1: [P(3), Z, P(3)], 2: [P(3)] * 4}),
    # frame 0: ANA (K/T/R/I: X) | CTN (L) ; frame 1: -AN | ACT | N-- ;
    # frame 2: --A | NAC (N/H/D/Y: X) | TN-
    'ambiguous': ([(0, 'ANACTN', 7)],
                  {0: [[7, 0, 0], Z], 1: [P(7), Z, P(7)], 2: [P(7), [7, 0, 0], P(7)]}),
    # one '-' with a fixed amino acid is a letter: frame 0 CT- (L) | GG- (G) ;
    # frame 1: -CT | -GG (R or G) | --- (1 own + 2 padding: blank) ; frame 2: --C | T-G | G--
    'one_dash_letter': ([(0, 'CT-GG-', 4)], {0: [Z, Z], 1: [P(4), P(4), Z], 2: [P(4)] * 3}),
    # frame 0: NNN (X) ; frame 1: -NN | N-- ; frame 2: --N | NN-
    'all_n': ([(0, 'NNN', 1)], {0: [[1, 0, 0]], 1: [P(1)] * 2, 2: [P(1)] * 2}),
    # counts add up per cell: codon 0 X = 2 + 3; the third row is a deletion of
    # codon 1 in frame 0 and blank in frames 1 and 2 (its '-' meet padding)
    'sums': ([(0, 'ANA', 2), (0, 'ANA', 3), (3, '---', 4)],
             {0: [[5, 0, 0], [0, 0, 4]], 1: [P(5), P(5), Z], 2: [P(5), P(5), Z]}),
}

"""The mate concordance without a device: the two command lines' new
arguments, the header variants of nuc_detail.csv, the reader of
concordance.csv and the sum a sharded job's rank 0 writes."""
import io
import os

import numpy as np

import concordance_cases as cases
import concordance_oracle as oracle
from micall_amd import aln2counts as a2c
from micall_amd import projects
from micall_amd import sam2aln as s2a


def _report():
    return a2c.SequenceReport(a2c.InsertionWriter(io.StringIO()), projects.ProjectConfig.loadDefault(),
                              a2c.CONSEQ_MIXTURE_CUTOFFS)


def test_sam2aln_command_line(monkeypatch, tmp_path):
    (tmp_path / 'r.csv').write_text('')
    files = [str(tmp_path / n) for n in ('r.csv', 'a.csv')]
    monkeypatch.setattr('sys.argv', ['sam2aln'] + files + ['--concordance_csv', str(tmp_path / 'c.csv'),
                                                           '--cycle_concordance_csv', str(tmp_path / 'y.csv')])
    a = s2a.parseArgs()
    assert a.concordance_csv.name == str(tmp_path / 'c.csv') and a.concordance_csv.mode == 'w'
    assert a.cycle_concordance_csv.name == str(tmp_path / 'y.csv') and a.cycle_concordance_csv.mode == 'w'
    monkeypatch.setattr('sys.argv', ['sam2aln'] + files)
    b = s2a.parseArgs()
    assert b.concordance_csv is None and b.cycle_concordance_csv is None
    for h in (a.remap_csv, a.aligned_csv, a.concordance_csv, a.cycle_concordance_csv, b.remap_csv,
              b.aligned_csv):
        h.close()


def test_aln2counts_command_line(tmp_path):
    for name in ('aligned.csv', 'concordance.csv'):
        (tmp_path / name).write_text('')
    files = [str(tmp_path / n) for n in ('aligned.csv', 'nuc.csv', 'amino.csv', 'ins.csv', 'conseq.csv')]
    a = a2c._arguments(files + ['--concordance_csv', str(tmp_path / 'concordance.csv')])
    assert a.concordance_csv.name == str(tmp_path / 'concordance.csv') and a.concordance_csv.mode == 'r'
    b = a2c._arguments(files)
    assert b.concordance_csv is None
    for h in (a.aligned_csv, a.nuc_csv, a.amino_csv, a.coord_ins_csv, a.conseq_csv, a.concordance_csv,
              b.aligned_csv, b.nuc_csv, b.amino_csv, b.coord_ins_csv, b.conseq_csv):
        h.close()


def test_nuc_detail_header_variants():
    base = 'seed,region,q-cutoff,query.nuc.pos,refseq.nuc.pos,A,C,G,T,N,del,clip,coverage'
    want = {(False, False): base, (True, False): base + ',ins',
            (False, True): base + ',overlap,mismatch,indel',
            (True, True): base + ',ins,overlap,mismatch,indel'}
    for (ins, conc), line in want.items():
        out = io.StringIO()
        _report().write_nuc_detail_header(out, ins, conc)
        assert out.getvalue() == line + os.linesep
    out = io.StringIO()
    _report().write_nuc_detail_header(out)              # as before this option
    assert out.getvalue() == base + os.linesep


def test_reader_of_concordance_csv():
    rows, want_p, want_r = cases.combined()
    text = cases.expected_texts(want_p, want_r)[0]
    got = a2c._read_concordance(io.StringIO(text))
    assert sorted(got) == ['R1', 'alpha', 'zeta']
    assert {(n, p): list(v) for n, at in got.items() for p, v in at.items()} == \
        {key: v[:3] for key, v in want_p.items()}
    assert a2c._read_concordance(io.StringIO('refname,pos,overlap,mismatch,indel,nocall,unresolved\n')) == {}
    quoted = a2c._read_concordance(io.StringIO(
        'refname,pos,overlap,mismatch,indel,nocall,unresolved\n"b,1",-3,7,2,1,0,1\n'))
    assert quoted == {'b,1': {-3: (7, 2, 1)}}


class _TwoRanks:
    """A job of two ranks seen from rank 0: the other rank's parts are given."""
    rank, world = 0, 2

    def __init__(self, other):
        self.other = list(other)

    def all_gather_bytes(self, mine):
        return [mine, self.other.pop(0)]


class _Counts:
    def __init__(self, names, positions, reads):
        ids = np.array([names.index(n) for n, _ in sorted(positions)], dtype=np.int32)
        pos = np.array([p for _, p in sorted(positions)], dtype=np.int64)
        cnt = np.array([positions[k] for k in sorted(positions)], dtype=np.int32).reshape(-1, 5)
        rd = np.array([[r, by == 'quality', v] + reads[r, by, v] for r, by, v in sorted(reads)],
                      dtype=np.int64).reshape(-1, 5)
        self.parts = ids, pos, cnt, rd

    def sam2aln_conc_counts(self):
        return self.parts


def test_sharded_sum_writes_the_whole_jobs_files():
    """Two ranks with half of the hand-written cases each, their names in
    different orders: rank 0 writes the files of all the cases together."""
    names = sorted(cases.CASES)
    halves = []
    for part, order in ((names[::2], ['R1', 'alpha', 'zeta']), (names[1::2], ['zeta', 'R1', 'alpha'])):
        text = cases.text([[n + '.' + r[0]] + r[1:] for n in part for r in cases.CASES[n][0]])
        halves.append((order, _Counts(order, *oracle.count(text))))
    (names0, mine), (names1, other) = halves
    ids, pos, cnt, rd = other.parts
    sh = _TwoRanks(['\n'.join(names1).encode(), ids.tobytes(), pos.tobytes(), cnt.tobytes(), rd.tobytes()])
    outs = io.StringIO(), io.StringIO()
    s2a._concordance_sharded(sh, mine, names0, *outs)
    rows, want_p, want_r = cases.combined()
    assert (outs[0].getvalue(), outs[1].getvalue()) == cases.expected_texts(want_p, want_r)

"""covariation.csv without a device: what aln2counts refuses before any device
work, the header, the measures and the command line."""
import io

import pytest

import covariation_cases as cases
import covariation_oracle as co
from micall_amd import aln2counts as a2c
from micall_amd import projects

BAD = [
    (dict(min_fraction=0), 'min_fraction'),
    (dict(min_fraction=-0.1), 'min_fraction'),
    (dict(min_fraction=1.01), 'min_fraction'),
    (dict(min_fraction='0.1'), 'min_fraction'),
    (dict(min_fraction=None), 'min_fraction'),
    (dict(min_fraction=True), 'min_fraction'),
    (dict(min_count=0), 'min_count'),
    (dict(min_count=-3), 'min_count'),
    (dict(min_count=1.5), 'min_count'),
    (dict(min_count=None), 'min_count'),
    (dict(max_variants=0), 'max_variants'),
    (dict(max_variants=257), 'max_variants'),
    (dict(max_variants=2.0), 'max_variants'),
]


def _report():
    return a2c.SequenceReport(a2c.InsertionWriter(io.StringIO()), projects.ProjectConfig.loadDefault(),
                              a2c.CONSEQ_MIXTURE_CUTOFFS)


def _call(**kw):
    outs = [io.StringIO() for _ in range(4)]
    a2c.aln2counts(io.StringIO('refname,qcut,rank,count,offset,seq\n'), *outs, **kw)
    return outs


@pytest.mark.parametrize('kw,name', BAD)
def test_bad_thresholds_are_refused_by_name(kw, name):
    with pytest.raises(ValueError, match='covariation: ' + name):
        _report().count_covariation(**kw)
    with pytest.raises(ValueError, match='covariation: ' + name):
        _report().write_covariation(io.StringIO(), **kw)
    with pytest.raises(ValueError, match='covariation: ' + name):
        _call(covariation_csv=io.StringIO(), **{'covariation_' + k: v for k, v in kw.items()})


def test_the_edges_of_the_ranges_are_accepted():
    assert a2c._check_covariation(1, 1, 1) == (1.0, 1, 1)
    assert a2c._check_covariation(1e-9, 10 ** 12, 256) == (1e-9, 10 ** 12, 256)
    assert a2c._check_covariation() == (0.01, 10, 256)
    assert a2c.COVARIATION_MAX_VARIANTS == 256


def test_a_report_that_read_nothing_counts_nothing():
    report = _report()
    assert report.count_covariation() == []
    assert report.covariation_stats == dict(variants=0, dropped=0, columns=0, pairs=0, native=None)


def test_header():
    out = io.StringIO()
    _report().write_covariation_header(out)
    assert out.getvalue().splitlines() == [
        'seed,q-cutoff,region.a,pos.a,aa.a,region.b,pos.b,aa.b,n,n.a,n.b,n.ab,direction,r2']
    assert out.getvalue().splitlines()[0].split(',') == co.HEADER


def test_the_called_characters_and_their_bits():
    assert a2c.COVARIATION_CALLED == co.CALLED
    assert a2c._COVAR_CALLED == co.CALLED_MASK
    assert a2c._COVAR_BIT == [1 << co.CODES.index(ch) for ch in co.CALLED]


@pytest.mark.parametrize('counts', sorted(cases.MEASURES))
def test_direction_and_r2(counts):
    assert (a2c.covariation_direction(*counts), a2c.covariation_r2(*counts)) == cases.MEASURES[counts]


def test_command_line(tmp_path):
    (tmp_path / 'aligned.csv').write_text('')
    files = [str(tmp_path / n) for n in ('aligned.csv', 'nuc.csv', 'amino.csv', 'ins.csv', 'conseq.csv')]
    a = a2c._arguments(files + ['--covariation_csv', str(tmp_path / 'covariation.csv'),
                                '--covariation_min_fraction', '0.05', '--covariation_min_count', '3',
                                '--covariation_max_variants', '64'])
    assert a.covariation_csv.name == str(tmp_path / 'covariation.csv') and a.covariation_csv.mode == 'w'
    assert (a.covariation_min_fraction, a.covariation_min_count, a.covariation_max_variants) == (0.05, 3, 64)
    b = a2c._arguments(files)
    assert b.covariation_csv is None
    assert (b.covariation_min_fraction, b.covariation_min_count, b.covariation_max_variants) == (0.01, 10, 256)
    for h in (a.aligned_csv, a.nuc_csv, a.amino_csv, a.coord_ins_csv, a.conseq_csv, a.covariation_csv,
              b.aligned_csv, b.nuc_csv, b.amino_csv, b.coord_ins_csv, b.conseq_csv):
        h.close()

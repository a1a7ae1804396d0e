"""linkage.csv without a device: what aln2counts refuses before any device
work, the header, the JSON file of positions and the command line."""
import io
import json

import pytest

import linkage_oracle as lo
from micall_amd import aln2counts as a2c
from micall_amd import projects

BAD_SETS = [
    ({'RT': [[]]}, 'RT, set 0'),
    ({'RT': [[41], list(range(1, 14))]}, 'RT, set 1'),
    ({'PR': [[30, 30]]}, 'PR, set 0'),
    ({'PR': [[46, 30]]}, 'PR, set 0'),
    ({'PR': [[10], [20], [0, 5]]}, 'PR, set 2'),
    ({'INT': [[-1]]}, 'INT, set 0'),
    ({'INT': [[1.5]]}, 'INT, set 0'),
    ({'INT': [['140']]}, 'INT, set 0'),
    ({'INT': [[True, 2]]}, 'INT, set 0'),
    ({'INT': [7]}, 'INT, set 0'),
]


def _report():
    return a2c.SequenceReport(a2c.InsertionWriter(io.StringIO()), projects.ProjectConfig.loadDefault(),
                              a2c.CONSEQ_MIXTURE_CUTOFFS)


def _call(**kw):
    outs = [io.StringIO() for _ in range(4)]
    a2c.aln2counts(io.StringIO('refname,qcut,rank,count,offset,seq\n'), *outs, **kw)
    return outs


@pytest.mark.parametrize('positions,where', BAD_SETS)
def test_bad_sets_are_refused_by_name(positions, where):
    with pytest.raises(ValueError, match=where):
        _report().count_linkage(positions)
    with pytest.raises(ValueError, match=where):
        _report().write_linkage(io.StringIO(), positions)
    with pytest.raises(ValueError, match=where):
        _call(linkage_csv=io.StringIO(), linkage_positions=positions)


def test_twelve_positions_are_accepted_thirteen_are_not():
    assert a2c._check_linkage({'RT': [list(range(1, 13))]}) == {'RT': [list(range(1, 13))]}
    with pytest.raises(ValueError, match='more than 12'):
        a2c._check_linkage({'RT': [list(range(1, 14))]})


@pytest.mark.parametrize('min_count', [0, -1, 1.5, None])
def test_min_count_below_one_is_refused(min_count):
    with pytest.raises(ValueError, match='min_count'):
        _report().count_linkage({'RT': [[41]]}, min_count)
    with pytest.raises(ValueError, match='min_count'):
        _call(linkage_csv=io.StringIO(), linkage_positions={'RT': [[41]]}, linkage_min_count=min_count)


def test_linkage_csv_needs_positions():
    with pytest.raises(ValueError, match='linkage_positions'):
        _call(linkage_csv=io.StringIO())


def test_a_position_past_the_reference_is_refused_when_the_region_is_met():
    """PR has 99 positions: [99] is a set, [100] is refused once a run has
    PR among its coordinate regions -- and not before, nor for a region the
    seed does not have."""
    report = _report()
    report.coordinate_refs = {'PR': 'P' * 99}
    report._coord_maps = {}
    assert report.count_linkage({'PR': [[30, 99]], 'RT': [[4000]]}) == []
    with pytest.raises(ValueError, match='PR, set 1'):
        report.count_linkage({'PR': [[30, 99], [99, 100]]})
    assert _report().count_linkage({'PR': [[100]]}) == []


def test_positions_from_a_json_file(tmp_path):
    path = tmp_path / 'positions.json'
    path.write_text(json.dumps({'RT': [[41, 67, 70], [184, 215, 219]]}))
    assert a2c._check_linkage(a2c._load_linkage(str(path))) == {'RT': [[41, 67, 70], [184, 215, 219]]}
    path.write_text(json.dumps({'RT': [[41, 41]]}))
    with pytest.raises(ValueError, match='RT, set 0'):
        _call(linkage_csv=io.StringIO(), linkage_positions=str(path))


def test_header():
    out = io.StringIO()
    _report().write_linkage_header(out)
    assert out.getvalue().splitlines() == ['seed,region,q-cutoff,positions,haplotype,count,coverage']
    assert out.getvalue().splitlines()[0].split(',') == lo.HEADER


def test_command_line(tmp_path):
    for name in ('aligned.csv', 'positions.json'):
        (tmp_path / name).write_text('')
    files = [str(tmp_path / n) for n in ('aligned.csv', 'nuc.csv', 'amino.csv', 'ins.csv', 'conseq.csv')]
    a = a2c._arguments(files + ['--linkage_csv', str(tmp_path / 'linkage.csv'), '--linkage_positions',
                                str(tmp_path / 'positions.json'), '--linkage_min_count', '3'])
    assert a.linkage_csv.name == str(tmp_path / 'linkage.csv') and a.linkage_csv.mode == 'w'
    assert a.linkage_positions == str(tmp_path / 'positions.json') and a.linkage_min_count == 3
    b = a2c._arguments(files)
    assert b.linkage_csv is None and b.linkage_positions is None and b.linkage_min_count == 1
    for h in (a.aligned_csv, a.nuc_csv, a.amino_csv, a.coord_ins_csv, a.conseq_csv, a.linkage_csv,
              b.aligned_csv, b.nuc_csv, b.amino_csv, b.coord_ins_csv, b.conseq_csv):
        h.close()

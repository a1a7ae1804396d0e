"""The nucleotide variant report without a device: the plain-Python
restatement (tests/variants_cases.py) pinned to the reference's twelve
variant tests through the oracle's coordinate mapping, the window rule, and
ProjectConfig.getMaxVariants."""
import io
import json

import pytest

import a2c_replay
import og_aln2counts as og
import variants_cases as vc
from micall_amd import aln2counts as a2c
from micall_amd import projects

ORACLE = dict(SequenceReport=og.Report, InsertionWriter=og.Inserts, projects=og.Projects)
WINDOWS = [([], (0, 0)), ([-1, -1, -1], (0, 0)), ([-1, 2, 3, -1], (6, 12)), ([0, 1], (0, 6)),
           ([0], (0, 0)), ([-1, 0, -1], (0, 0))]


def test_twelve_reference_cases_are_recorded():
    assert len(vc.EXPECTED) == 12 and set(vc.SCRIPTS) == set(vc.EXPECTED)


@pytest.mark.parametrize('test', sorted(vc.EXPECTED))
def test_restatement_reproduces_reference_texts(test):
    assert vc.replay(test, ORACLE, vc.oracle_write) == vc.EXPECTED[test]


@pytest.mark.parametrize('index,want', WINDOWS)
def test_window_rule(index, want):
    assert vc.variant_window(index) == want
    assert a2c._variant_window(index) == want


def _recorded_configs():
    configs = {}
    for script in a2c_replay.scripts():
        for call in script['calls']:
            if call['op'] == 'read':
                configs[json.dumps(call['config'], sort_keys=True)] = call['config']
    return list(configs.values())


def test_get_max_variants_of_recorded_configs():
    seen = set()
    for cfg in _recorded_configs():
        conf = projects.ProjectConfig.from_config(cfg)
        for project in cfg['projects'].values():
            for entry in project['regions']:
                name = entry['coordinate_region']
                assert conf.getMaxVariants(name) == vc.max_variants_of(cfg, name)
                seen.add(conf.getMaxVariants(name))
        assert conf.getMaxVariants('no such region') == 0
    assert {10, 3, 2} <= seen


def test_get_max_variants_takes_the_largest_project():
    cfg = {'projects': {'P1': {'max_variants': 4, 'regions': [
                            {'coordinate_region': 'R1', 'seed_region_names': ['S']}]},
                        'P2': {'max_variants': 7, 'regions': [
                            {'coordinate_region': 'R1', 'seed_region_names': ['S']},
                            {'coordinate_region': 'R2', 'seed_region_names': ['S']}]},
                        'P3': {'regions': [{'coordinate_region': 'R3', 'seed_region_names': ['S']}]}},
           'regions': {'S': {'reference': ['AAATTT']}, 'R1': {'reference': ['KF']},
                       'R2': {'reference': ['KF']}, 'R3': {'reference': ['KF']}}}
    conf = projects.ProjectConfig.from_config(cfg)
    assert [conf.getMaxVariants(r) for r in ('R1', 'R2', 'R3', 'R4')] == [7, 7, 0, 0]
    loaded = projects.ProjectConfig()
    loaded.load(io.StringIO(json.dumps(cfg)))
    assert loaded.getMaxVariants('R1') == 7


def test_get_max_variants_defaults():
    conf = projects.ProjectConfig.loadDefault()
    assert conf.getMaxVariants('HLA-B-exon2') == 10 and conf.getMaxVariants('HLA-B-exon3') == 10
    assert conf.getMaxVariants('PR') == 0 and conf.getMaxVariants('RT') == 0
    assert 'PR' in conf.regions and 'RT' in conf.regions


def test_restatement_rules():
    rows = [dict(seq='AAATTT', offset=0, count=3), dict(seq='TTT', offset=3, count=2),
            dict(seq='---TTT', offset=0, count=4), dict(seq='AAATTn', offset=0, count=1),
            dict(seq='AAATTN', offset=0, count=1), dict(seq='AAATT', offset=0, count=1)]
    # padding dashes equal sequence dashes; n is not N; a prefix sorts below
    assert vc.expected_variants(rows, 0, 6, 4, 9) == [
        (6, '---TTT'), (3, 'AAATTT'), (1, 'AAATTn'), (1, 'AAATTN'), (1, 'AAATT')]
    # 2 * 3 == 6 is rejected, 2 * 3 > 5 is kept
    assert vc.expected_variants(rows[1:2], 0, 6, 6, 9) == []
    assert vc.expected_variants(rows[1:2], 0, 6, 5, 9) == [(2, '---TTT')]
    assert vc.expected_variants(rows, 0, 6, 4, 0) == []
    assert vc.tie_at_cut(rows, 0, 6, 4, 3) and not vc.tie_at_cut(rows, 0, 6, 4, 2)

"""aln2counts' linkage.csv: the amino acids single reads link at chosen
positions, counted on the device (k_a2c_link / k_a2c_tab_count /
k_a2c_link_compact through mh_a2c_link; SequenceReport.count_linkage,
aln2counts(linkage_csv=)).

1. The device call against tests/linkage_oracle.py on rows loaded with
   a2c_load_rows, compared exactly -- entries, order, coverage: the
   hand-worked cases, the key's width, row edges, frames and bins, the pass
   boundary, counts above 2**31, chunk edges, random rows, min_count.
2. The file against the oracle's, built from og_aln2counts.Report's map; the
   one-position sets against amino_detail.csv; the resident chain; two ranks.

A pass of the library holds at most 16 sets (four key bits) and at most 64
(set, position) slots (the lanes of a wave), whichever fills first."""
import csv
import gzip
import io
import json
import os
import random
import socket
import subprocess
import sys

import pytest

import linkage_cases
import linkage_oracle as lo
import og_aln2counts as og
from micall_amd import _native, session
from micall_amd import aln2counts as a2c
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
WORKER = os.path.join(HERE, 'gpu_linkage_worker.py')
SLOT = 2
PASS_SETS, PASS_SLOTS = 16, 64
POSITIONS = {'RT': [[41, 67, 70], [184, 215, 219], [41, 215]], 'PR': [[30, 46, 82, 84, 90]],
             'INT': [[140, 148, 155]]}
PLAIN = ('nuc', 'amino', 'coord_ins', 'conseq')
SHIFTED = 'syn_pol_indel+1'
_EXPECTED = {}


# ---------------------------------------------------------------------------
# 1. the device call against the oracle
# ---------------------------------------------------------------------------
def _load(groups, slot=SLOT):
    ctx = session.context()
    rows = [r for grp in groups for r in grp]
    first = [0]
    for grp in groups:
        first.append(first[-1] + len(grp))
    ctx.a2c_load_rows(slot, [r[1] for r in rows], [r[0] for r in rows], [r[2] for r in rows], first,
                      a2c._CODON_CHARS)
    return ctx


def _check(rows, sets, min_count=1, groups=None, g=0):
    """mh_a2c_link over group g (rows) against the oracle; returns (entries,
    stats)."""
    ctx = _load(groups or [rows])
    got, stats = ctx.a2c_link(SLOT, g, sets, min_count)
    want, coverage = lo.entries(rows, sets, min_count)
    assert got == want
    assert stats['coverage'] == coverage
    assert stats['fetched'] == len(want)
    assert stats['entries'] == len(lo.entries(rows, sets, 1)[0])
    return got, stats


def _codon_of_each_character():
    """A codon text for each of the 24 haplotype characters."""
    found = {}
    for a in 'ACGT':
        for b in 'ACGT':
            for c in 'ACGT':
                found.setdefault(og.translate(a + b + c), a + b + c)
    assert sorted(found) == sorted(og.AMINOS)
    found.update({'X': 'ANA', '?': 'A-A', '-': '---'})
    return found


@pytest.mark.parametrize('name', sorted(linkage_cases.CASES))
def test_hand_worked_cases(name):
    rows, sets, min_count, entries, coverage = linkage_cases.CASES[name]
    got, stats = _check(rows, sets, min_count)
    assert got == entries and stats['coverage'] == coverage


def test_key_width():
    """Sets of 1, 2, 11 and 12 codons, and each of the 24 characters at the
    last position of a 12-set (the key's top code field), the 12-set given
    five times so that it also sits last in a full pass of 60 slots."""
    codon = _codon_of_each_character()
    assert len(codon) == 24
    rows = [(0, 'AAA' * 11 + text + 'CCC', 3 + k) for k, text in enumerate(codon.values())]
    sets = [(0, list(range(12)))] * 5 + [(0, [11]), (0, [10, 11]), (0, list(range(1, 12))), (0, list(range(12)))]
    got, stats = _check(rows, sets)
    last = {e[2][-1:].decode() for e in got if e[0] == 4}
    assert last == set(codon) and all(len(e[2]) == 12 for e in got if e[0] in (0, 4, 8))
    assert [e[1:] for e in got if e[0] == 0] == [e[1:] for e in got if e[0] == 4] == [e[1:] for e in got if e[0] == 8]
    assert stats['coverage'][5] == sum(r[2] for r in rows)


def test_thirteen_codons_are_refused():
    ctx = _load([[(0, 'AAA' * 14, 1)]])
    assert ctx.a2c_link(SLOT, 0, [(0, list(range(12)))])[0] == [(0, 1, b'K' * 12)]
    with pytest.raises(_native.NativeError):
        ctx.a2c_link(SLOT, 0, [(0, list(range(13)))])


def test_row_edges():
    # a row ending inside the set's last codon, a row starting inside its first
    got, _ = _check([(0, 'AAAGGGT', 2), (1, 'AAGGGTTT', 3)], [(0, [0, 1, 2])])
    assert got == [(0, 3, b'?GF'), (0, 2, b'KG?')]
    # offset % 3 + frame >= 3: the first codon the row reaches is padding only
    got, stats = _check([(2, 'GAAATTT', 1), (5, 'AAATTT', 2)], [(1, [0, 1]), (1, [1, 2]), (2, [1, 2]), (2, [2, 3])])
    assert stats['coverage'] == [0, 1, 1, 3]
    # three '-' of the row are a deletion, the padding's are blank
    got, stats = _check([(0, 'AAA---TTT', 4), (6, 'TTT', 1), (0, 'AAA', 2)], [(0, [1, 2]), (0, [0, 1])])
    assert got == [(0, 4, b'-F'), (1, 4, b'K-')] and stats['coverage'] == [4, 4]
    # 'nnn' is blank, 'nAn' is partial; TAA is '*', ANA is X
    got, stats = _check([(0, 'TAAnnnANA', 1), (0, 'TAAnAnANA', 2)], [(0, [0, 1, 2]), (0, [0, 2])])
    assert got == [(0, 2, b'*?X'), (1, 3, b'*X')] and stats['coverage'] == [2, 3]
    # a codon beyond every row, alone and in a set with one that is read
    got, stats = _check([(0, 'AAATTT', 5), (30, 'ACGT', 1)], [(0, [400]), (0, [0, 400]), (2, [2 ** 31 - 1])])
    assert got == [] and stats['coverage'] == [0, 0, 0] and stats['pairs'] == 0 and stats['entries'] == 0


def test_frames_and_bins():
    """Frames 0, 1 and 2 in one call; codons 20 | 21 and 41 | 42 are the last
    of one 21-codon bin and the first of the next; a set over three bins."""
    rng = random.Random(3)
    rows = [(rng.choice((0, 1, 2, 57, 60, 61, 120)), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(3, 160))),
             rng.randint(1, 9)) for _ in range(300)]
    rows += [(0, ''.join(rng.choice('ACGT') for _ in range(150)), 7), (1, 'ACGTTGCA' * 19, 5), (2, 'CCGATA' * 25, 3)]
    sets = [(0, [20, 21]), (1, [20, 21]), (2, [20, 21]), (0, [41, 42]), (1, [41, 42]), (2, [41, 42]),
            (0, [5, 30, 50]), (1, [5, 30, 50]), (2, [0, 20, 21, 41, 42, 49]), (0, [20]), (0, [21]), (1, [42])]
    got, stats = _check(rows, sets)
    assert all(c > 0 for c in stats['coverage'])
    assert {e[0] for e in got} == set(range(len(sets)))


def _many_sets(n, rng, top=40):
    return [(rng.randrange(3), sorted(rng.sample(range(top), rng.randint(1, 3)))) for _ in range(n)]


@pytest.mark.parametrize('n_sets', [16, 17, 33])
def test_pass_boundary(n_sets):
    """16 sets fill a pass, the 17th and the 33rd open another."""
    rng = random.Random(n_sets)
    rows = [(rng.randint(0, 30), ''.join(rng.choice('ACGT') for _ in range(rng.randint(100, 160))), rng.randint(1, 9))
            for _ in range(150)]
    sets = _many_sets(n_sets, rng)
    assert sum(len(s[1]) for s in sets[:PASS_SETS]) <= PASS_SLOTS
    got, _ = _check(rows, sets)
    assert {e[0] for e in got} == set(range(n_sets))


def test_slots_fill_a_pass_before_sets():
    """Six 12-sets are 72 slots: the sixth goes in a second pass."""
    rng = random.Random(6)
    rows = [(0, ''.join(rng.choice('AC') for _ in range(60)), rng.randint(1, 9)) for _ in range(100)]
    sets = [(f % 3, list(range(k, k + 12))) for f, k in enumerate((0, 1, 2, 3, 4, 5))]
    assert sum(len(s[1]) for s in sets[:5]) <= PASS_SLOTS < sum(len(s[1]) for s in sets)
    got, _ = _check(rows, sets)
    assert {e[0] for e in got} == set(range(6))


def test_equal_strings_and_repeated_sets():
    rows = [(0, 'AAAAAATTTTTT', 3), (0, 'AAAAAATTT', 2), (0, 'GGGGGGTTTTTT', 1)]
    # two different sets with the same haplotype strings stay apart
    got, _ = _check(rows, [(0, [0, 2]), (0, [1, 2])])
    assert got == [(0, 5, b'KF'), (0, 1, b'GF'), (1, 5, b'KF'), (1, 1, b'GF')]
    # the same set twice, in one pass and across two
    got, _ = _check(rows, [(0, [0, 3])] * 2)
    assert got == [(0, 3, b'KF'), (0, 1, b'GF'), (1, 3, b'KF'), (1, 1, b'GF')]
    got, _ = _check(rows, [(0, [0, 3])] + [(0, [1])] * 15 + [(0, [0, 3])])
    assert [e[1:] for e in got if e[0] == 0] == [e[1:] for e in got if e[0] == 16] == [(3, b'KF'), (1, b'GF')]


def test_one_entry_above_two_to_the_31():
    rows = [(0, 'AAATTT', 600000)] * 5000
    got, stats = _check(rows, [(0, [0, 1])])
    assert got == [(0, 3000000000, b'KF')] and got[0][1] > 2 ** 31
    assert stats['coverage'] == [3000000000] and stats['pairs'] == 5000 and stats['entries'] == 1


def test_seventy_haplotypes_in_one_wave():
    """More distinct keys among 64 consecutive pairs than the wave combines
    (four rounds): the rest go to the table lane by lane."""
    letters = [c for c in _codon_of_each_character().values() if '-' not in c and 'N' not in c]
    rows = [(0, letters[k % 21] + letters[k // 21], 1 + k % 5) for k in range(70)]
    got, stats = _check(rows + rows[:10], [(0, [0, 1])])
    assert stats['entries'] == 70 and len(got) == 70


@pytest.mark.parametrize('n', [1025, 2049])
def test_chunk_edges(n):
    rng = random.Random(n)
    rows = [(rng.randrange(0, 12), ''.join(rng.choice('ACGTN-n') for _ in range(rng.randint(1, 40))), rng.randint(1, 9))
            for _ in range(n)]
    _check(rows, [(0, [2, 5]), (1, [4]), (2, [3, 4, 6])])


def _random_case():
    rng = random.Random(20)
    rows = [(rng.choice((0, 1, 2, 7, 30, 31)) + rng.randrange(0, 3) * 3,
             ''.join(rng.choice('ACGTN-n') for _ in range(rng.choice((5, 40, 90, 151)))), rng.randint(1, 4))
            for _ in range(4000)]
    sets = [(rng.randrange(3), sorted(rng.sample(range(45), rng.choice((1, 1, 2, 2, 3, 5, 12))))) for _ in range(20)]
    return rows, sets


def test_random_rows():
    rows, sets = _random_case()
    # by the oracle alone: a set with entries on both sides of the cut, a tie in count
    everything = lo.entries(rows, sets, 1)[0]
    per_set = {}
    for s, n, _h in everything:
        per_set.setdefault(s, []).append(n)
    assert any(min(c) < 3 <= max(c) for c in per_set.values())
    assert any(len(set(c)) < len(c) for c in per_set.values())
    assert any(len(s[1]) == 12 for s in sets)
    for min_count in (1, 3):
        _check(rows, sets, min_count)


def test_min_count_keeps_coverage_and_fetches_less():
    rows = [(0, 'AAATTT', 5), (0, 'AGATTT', 2), (0, 'ACATTT', 1), (0, 'ANATTT', 1), (0, 'AAATTC', 1)]
    got, stats = _check(rows, [(0, [0, 1]), (0, [0])], 2)
    assert got == [(0, 6, b'KF'), (0, 2, b'RF'), (1, 6, b'K'), (1, 2, b'R')]
    assert stats['fetched'] == 4 and stats['entries'] == 8 and stats['pairs'] == 10
    assert stats['coverage'] == [10, 10]


def test_second_group_of_a_slot():
    first = [(0, 'GGGGGGGGG', 9)] * 3
    second = [(3, 'AAATTT', 2), (0, 'CCCAAATTT', 1), (3, 'AGA', 4)]
    got, _ = _check(second, [(0, [1, 2]), (0, [0])], groups=[first, second], g=1)
    assert got == [(0, 3, b'KF'), (1, 1, b'P')]
    got, _ = _check(first, [(0, [1, 2])], groups=[first, second], g=0)
    assert got == [(0, 27, b'GG')]


def test_bad_requests_are_refused():
    ctx = _load([[(0, 'AAATTT', 1)]])
    ok = [(0, [0, 1])]
    assert ctx.a2c_link(SLOT, 0, ok)[0] == [(0, 1, b'KF')]
    for sets, min_count in (([], 1), ([(0, [])], 1), ([(0, list(range(13)))], 1), ([(3, [0])], 1),
                            ([(-1, [0])], 1), ([(0, [0, -1])], 1), (ok, 0), (ok, -5)):
        with pytest.raises(_native.NativeError):
            ctx.a2c_link(SLOT, 0, sets, min_count)
    for g in (1, -1):
        with pytest.raises(_native.NativeError, match='no group'):
            ctx.a2c_link(SLOT, g, ok)
    # the entries of a refused call are gone, and so are those of the call before
    assert ctx.a2c_link(SLOT, 0, ok)[0] == [(0, 1, b'KF')]
    # a load that failed leaves the slot without one
    with pytest.raises(_native.NativeError):
        ctx.a2c_load_rows(SLOT, ['AXA'], [0], [1], [0, 1], a2c._CODON_CHARS)
    with pytest.raises(_native.NativeError, match='nothing is loaded'):
        ctx.a2c_link(SLOT, 0, ok)


# ---------------------------------------------------------------------------
# 2. the file
# ---------------------------------------------------------------------------
def _gz(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.csv.gz'), 'rt') as f:
        return f.read()


def _rows(text):
    return list(csv.reader(io.StringIO(text)))


def _aligned(case):
    """The golden aligned.csv; SHIFTED is syn_pol_indel's with every offset
    one further right, as tests/test_gpu_amino_detail.py builds it: its
    regions read in frame 2 (the goldens' own all sit in frame 0)."""
    if case == SHIFTED:
        rows = _rows(_aligned('syn_pol_indel'))
        k = rows[0].index('offset')
        out = io.StringIO()
        csv.writer(out, lineterminator='\n').writerows(
            [rows[0]] + [r[:k] + [int(r[k]) + 1] + r[k + 1:] for r in rows[1:]])
        return out.getvalue()
    return _gz(case, 'aligned')


def _expected(case, min_count=1):
    if (case, min_count) not in _EXPECTED:
        _EXPECTED[case, min_count] = lo.expected(_aligned(case), POSITIONS, min_count)
    return _EXPECTED[case, min_count]


def _file(lines):
    out = io.StringIO()
    csv.writer(out, lineterminator=os.linesep).writerows([lo.HEADER] + lines)
    return out.getvalue()


def _run(aligned_handle, linkage=True, positions=POSITIONS, **kw):
    outs = {k: io.StringIO() for k in PLAIN + ('linkage', 'amino_detail')}
    if linkage:
        kw.update(linkage_csv=outs['linkage'], linkage_positions=positions)
    if kw.pop('detail', False):
        kw['amino_detail_csv'] = outs['amino_detail']
    a2c.aln2counts(aligned_handle, outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'], **kw)
    return {k: v.getvalue() for k, v in outs.items()}


@pytest.mark.parametrize('case', ['syn_pol_indel', SHIFTED])
def test_linkage_file_matches_the_oracle(case, tmp_path):
    aligned = _aligned(case)
    lines, unplaced, tallies = _expected(case)
    # what the input must hold, by the oracle alone, for the comparison to mean something
    assert not unplaced and len(tallies) == 5
    assert sum(len(found) >= 2 for found, _ in tallies.values()) >= 4
    cover = {(region, s): c for (_seed, _q, region, s), (_f, c) in tallies.items()}
    assert 0 < cover['RT', 2] < cover['RT', 0]
    got = _run(io.StringIO(aligned))
    assert got['linkage'] == _file(lines)
    assert got['linkage'].count(os.linesep) == len(lines) + 1 > 40
    plain = _run(io.StringIO(aligned), linkage=False)
    assert all(got[k] == plain[k] for k in PLAIN) and plain['linkage'] == ''
    # min_count and the JSON file of positions
    path = tmp_path / 'positions.json'
    path.write_text(json.dumps(POSITIONS))
    cut = _run(io.StringIO(aligned), positions=str(path), linkage_min_count=4)
    assert cut['linkage'] == _file(_expected(case, 4)[0])
    assert 1 < cut['linkage'].count(os.linesep) < got['linkage'].count(os.linesep)


def test_the_shifted_case_reads_in_another_frame():
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    import amino_detail_oracle as ado
    rep.read(ado.groups(_aligned(SHIFTED))[0])
    assert set(rep.reading_frames.values()) == {2}


def test_sequence_report_lists_unplaced_sets_and_ignores_other_regions():
    """The third of syn_pol_indel's rows that end first: the consensus stops
    inside RT, so its later positions have no codon, and no frame aligns to
    INT (a failed.csv row)."""
    import amino_detail_oracle as ado
    report = a2c.SequenceReport(a2c.InsertionWriter(io.StringIO()), a2c.project_config.ProjectConfig.loadDefault(),
                                a2c.CONSEQ_MIXTURE_CUTOFFS)
    group = ado.groups(_aligned('syn_pol_indel'))[0]
    ends = sorted(int(r['offset']) + len(r['seq']) for r in group)
    group = [r for r in group if int(r['offset']) + len(r['seq']) <= ends[len(ends) // 3]]
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    rep.read(group)
    assert rep.reports['INT'] == [] and lo.place(rep, 'RT', [300]) is None and lo.place(rep, 'RT', [41, 300]) is None
    report.read(group)
    asked = {'RT': [[41, 67, 70], [300], [41, 300]], 'INT': [[140, 148, 155]], 'V3LOOP': [[1, 2]], 'nowhere': [[5]]}
    found = report.count_linkage(asked)
    assert [(f[0], f[1], f[2]) for f in found] == [('RT', 0, [41, 67, 70])]
    want, coverage = lo.count(group, *lo.place(rep, 'RT', [41, 67, 70]))
    assert found[0][3] == lo.ordered(want) and found[0][4] == coverage > 0
    assert report.linkage_unplaced == [('RT', 1), ('RT', 2)]
    out = io.StringIO()
    report.write_linkage(out, asked)
    assert _rows(out.getvalue()) == [[report.seed, 'RT', report.qcut, '41;67;70', h, str(n), str(coverage)]
                                     for h, n in lo.ordered(want)]
    with pytest.raises(ValueError, match='RT, set 0'):
        report.count_linkage({'RT': [[len(report.coordinate_refs['RT']) + 1]]})


def test_one_position_sets_are_amino_detail_rows():
    """All 99 PR positions as 99 one-position sets, with amino_detail_csv in
    the same call: every set's characters and coverage are its
    amino_detail.csv row (k_a2c_link against k_a2c_count and k_a2c_detail),
    over seven passes."""
    got = _run(io.StringIO(_aligned('syn_pol_indel')), positions={'PR': [[p] for p in range(1, 100)]}, detail=True)
    # (amino.csv carries one row past the reference's 99 positions, without a query position)
    detail = [r for r in _rows(got['amino_detail'])[1:] if r[1] == 'PR' and int(r[4]) <= 99]
    assert len(detail) == 99
    linked = {}
    for seed, region, qcut, where, hap, count, coverage in _rows(got['linkage'])[1:]:
        linked.setdefault(int(where), ({}, int(coverage)))[0][hap] = int(count)
    names = list(og.AMINOS) + ['X', '?', '-']
    checked = 0
    for r in detail:
        counts = {names[k]: int(x) for k, x in enumerate(r[5:29]) if int(x)}
        if r[3] == '':
            assert int(r[4]) not in linked
            continue
        found, coverage = linked.get(int(r[4]), ({}, 0))
        assert found == counts and coverage == int(r[31]), r[4]
        checked += bool(counts)
    assert checked > 90
    assert sum('?' in f for f, _ in linked.values()) > 5 and sum('X' in f for f, _ in linked.values()) > 20


def test_chain_linkage_from_the_device_rows_and_from_the_file(tmp_path, monkeypatch):
    d = os.path.join(E2E_DIR, 'syn_pol')
    r1, r2 = os.path.join(d, 'R1.fastq.gz'), os.path.join(d, 'R2.fastq.gz')
    prelim, remap_csv, aligned = (tmp_path / n for n in ('prelim.csv', 'remap.csv', 'aligned.csv'))
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    with open(prelim) as f, open(remap_csv, 'w') as out, open(tmp_path / 'counts.csv', 'w') as cn:
        rm.remap(r1, r2, f, out, cn, gzip=True, work_path=str(tmp_path))
    with open(remap_csv) as f, open(aligned, 'w') as out:
        s2a.sam2aln(f, out)
    with open(aligned) as f:
        dev = _run(f)
    assert session.stats['aln2counts_source'] == 'device'
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    with open(aligned) as f:
        csv_way = _run(f)
    assert session.stats['aln2counts_source'] == 'csv'
    assert dev == csv_way
    assert dev['linkage'].count(os.linesep) > 5


# ---------------------------------------------------------------------------
# 3. two ranks
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _with_a_split_haplotype():
    """syn_pol_indel's aligned.csv with one more row in front and one at the
    end: copies, at count 1, of a row that covers RT 41, 67 and 70 with
    codon 41 turned into TGG.  The new haplotype has count 1 in the first
    rank's share and 1 in the last's."""
    import amino_detail_oracle as ado
    text = _aligned('syn_pol_indel')
    group = ado.groups(text)[0]
    rep = og.Report(og.Inserts(io.StringIO()), og.default_projects(), og.CUTOFFS)
    rep.read(group)
    frame, codons = lo.place(rep, 'RT', [41, 67, 70])
    row = next(r for r in group if lo.haplotype(int(r['offset']), r['seq'], frame, codons) is not None and
               3 * codons[0] - frame - int(r['offset']) >= 0)
    at = 3 * codons[0] - frame - int(row['offset'])
    seq = row['seq'][:at] + 'TGG' + row['seq'][at + 3:]
    new = lo.haplotype(int(row['offset']), seq, frame, codons)
    assert new.startswith('W') and new not in lo.count(group, frame, codons)[0]
    head, body = text.split('\n', 1)
    line = ','.join([row['refname'], row['qcut'], '0', '1', row['offset'], seq]) + '\n'
    assert head.split(',') == ['refname', 'qcut', 'rank', 'count', 'offset', 'seq'] and body.endswith('\n')
    return head + '\n' + line + body + line, new


@pytest.mark.timeout(300)
def test_two_ranks_write_the_single_process_file(tmp_path):
    import amino_detail_oracle as ado
    split_text, new = _with_a_split_haplotype()
    # by the oracle: the new haplotype counts 1 without either of its rows and 2 with both
    want2 = lo.expected(split_text, POSITIONS, 2)
    rows = ado.groups(split_text)[0]
    assert len(ado.groups(split_text)) == 1
    key = (rows[0]['refname'], rows[0]['qcut'], 'RT', 0)
    assert want2[2][key][0][new] == 2
    assert [r[4] for r in want2[0] if r[3] == '41;67;70'].count(new) == 1
    one = lo.expected(split_text.rsplit('\n', 2)[0] + '\n', POSITIONS, 1)
    assert one[2][key][0][new] == 1
    cases = {'both_indel': dict(aligned=_aligned('syn_pol_indel'), min_count=1),
             'rank0_indel': dict(aligned=_aligned('syn_pol_indel'), min_count=1),
             'both_split_haplotype': dict(aligned=split_text, min_count=2)}
    root = tmp_path / 'cases'
    want = {}
    for name, case in cases.items():
        os.makedirs(root / name)
        (root / name / 'aligned.csv').write_text(case['aligned'])
        (root / name / 'linkage.json').write_text(json.dumps(dict(positions=POSITIONS, min_count=case['min_count'])))
        want[name] = _run(io.StringIO(case['aligned']), linkage_min_count=case['min_count'])
    assert want['both_indel']['linkage'] == _file(_expected('syn_pol_indel')[0])
    assert want['both_split_haplotype']['linkage'] == _file(want2[0])
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, WORKER, '--cases', str(root)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    stats = [json.load(open(root / ('rank%d.json' % r))) for r in range(2)]
    for name in cases:
        assert [s[name].get('mode') for s in stats] == ['sharded'] * 2, name
        n = [s[name]['rows'] for s in stats]
        assert min(n) >= 1 and max(n) < sum(n), (name, n)
        for k in PLAIN + ('linkage',):
            with open(root / name / (k + '.csv'), newline='') as f:
                assert f.read() == want[name][k], (name, k)

"""The nucleotide variant report on the device (mh_a2c_variants,
k_a2c_var_* in csrc/mh_a2c.hip; SequenceReport.count_variants /
write_variants, aln2counts(variants_csv=)): the reference's twelve variant
tests, whose expected texts the reference itself cannot write
(aln2counts.py:537-549 fails under Python 3), directed windows and a random
case against the plain-Python restatement (tests/variants_cases.py), the
collision path, the drop-in, the resident chain and a two-rank job."""
import gzip
import io
import json
import os
import random
import socket
import subprocess
import sys

import pytest

import og_aln2counts as og
import variants_cases as vc
from micall_amd import _native, projects, session
from micall_amd import aln2counts as a2c
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'gpu_variants_worker.py')
SLOT = 2
PRODUCT = dict(SequenceReport=a2c.SequenceReport, InsertionWriter=a2c.InsertionWriter,
               projects=projects.ProjectConfig.from_config)
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'failed', 'coverage')


# ---------------------------------------------------------------------------
# 1. the reference's twelve cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('test', sorted(vc.EXPECTED))
def test_reference_variant_cases(test):
    got = vc.replay(test, PRODUCT, lambda report, out, rows, config: report.write_variants(out))
    assert got == vc.EXPECTED[test]


# ---------------------------------------------------------------------------
# 2. directed windows against the restatement
# ---------------------------------------------------------------------------
def _row(seq, offset=0, count=1):
    return dict(seq=seq, offset=offset, count=count)


def _seq(rng, n, alphabet='ACGT'):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def _device(groups, g, regions, key_bits=64):
    """mh_a2c_variants over group g of the row groups, regions = [(start,
    end, ref_len, max_variants)]: (entries, stats)."""
    ctx = session.context()
    rows = [r for grp in groups for r in grp]
    first = [0]
    for grp in groups:
        first.append(first[-1] + len(grp))
    ctx.a2c_load_rows(SLOT, [r['seq'] for r in rows], [r['offset'] for r in rows],
                      [r['count'] for r in rows], first, a2c._CODON_CHARS)
    return ctx.a2c_variants(SLOT, g, *zip(*regions), key_bits=key_bits)


def _want(rows, regions):
    return [(k, n, s.encode()) for k, region in enumerate(regions)
            for n, s in vc.expected_variants(rows, *region)]


def _check(groups, g, regions):
    got, stats = _device(groups, g, regions)
    want = _want(groups[g], regions)
    assert got == want
    if all(r[3] <= 64 for r in regions):
        # only the kept sequences' text came to the host
        assert stats['text_bytes'] == sum(len(s) for _, _, s in want)
    return got, stats


def _family(rng, n_rows=60, length=3200):
    """Rows cut from one base sequence at several offsets and lengths, with
    substitutions, 'N', 'n' and '-' here and there; some repeated."""
    base = _seq(rng, length)
    rows = []
    for _ in range(n_rows):
        off = rng.choice([0, 0, 0, 40, 90, 100, 130, 400])
        s = list(base[off:max(off + 30, rng.choice([length, length, 500, 350, 3050, 170]))])
        for _ in range(rng.randrange(3)):
            s[rng.randrange(len(s))] = rng.choice('ACGTNn-')
        rows.append(_row(''.join(s), off, rng.randint(1, 9)))
    return rows + rows[:10]


@pytest.mark.parametrize('width', [0, 1, 63, 64, 65, 255, 256, 257, 3000])
def test_window_widths(width):
    rows = _family(random.Random(width))
    got, _ = _check([rows], 0, [(100, 100 + width, 0, 64)])
    assert bool(got) == (width > 0)
    assert all(len(s) <= width for _, _, s in got)


def test_window_edges_and_identity():
    rows = [_row('ACGTACGTACGTACGTACGT', 30, 2),          # 0: the window starts in its padding
            _row('GGGGGGGGGG', 0, 3),                     # 1: ends inside the window
            _row('ACGTACGT', 500, 5),                     # 2: wholly after the window
            _row('TTTTTTTT', 0, 7),                       # 3: ends before the late window
            _row('TTT', 3, 2), _row('---TTT', 0, 4),      # 4, 5: padding and sequence dashes
            _row('AAATTn', 0, 1), _row('AAATTN', 0, 1),   # 6, 7: n is not N
            _row('AAATT', 0, 1), _row('AAATTC', 0, 1)]    # 8, 9: a proper prefix of another
    regions = [(10, 50, 0, 64), (0, 6, 0, 64), (100, 200, 0, 64), (498, 503, 0, 64)]
    got, _ = _check([rows], 0, regions)
    assert (0, 2, b'-' * 20 + b'ACGTACGTACGTACGTACGT') in got
    assert (1, 6, b'---TTT') in got
    assert (1, 7, b'TTTTTT') in got and (1, 3, b'GGGGGG') in got
    tail = [e for e in got if e[0] == 1 and e[1] == 1]
    assert tail == [(1, 1, b'AAATTn'), (1, 1, b'AAATTN'), (1, 1, b'AAATTC'), (1, 1, b'AAATT')]
    assert not [e for e in got if e[0] == 2]              # '' and all-dash windows never count
    assert [e for e in got if e[0] == 3] == [(3, 5, b'--ACG')]


def test_filter_boundary():
    rows = [_row('ACG' + '-' * 5, 2, 1), _row('ACGT' + '-' * 4, 2, 1), _row('-' * 8, 2, 9)]
    # reference length 6: 2 * 3 == 6 is rejected, one more base is kept
    got, stats = _check([rows], 0, [(0, 10, 6, 64), (0, 10, 5, 64), (0, 10, 8, 64)])
    assert got == [(0, 1, b'--ACGT----'), (1, 1, b'--ACGT----'), (1, 1, b'--ACG-----')]
    assert stats['pairs'] == 3 and stats['entries'] == 3


def test_one_string_from_many_rows():
    rng = random.Random(3)
    main, other = _seq(rng, 90), _seq(rng, 90)
    rows = [_row(main + _seq(rng, 10), 0, 600000) for _ in range(5000)]
    rows += [_row(other, 0, 5), _row(main[:80], 0, 1)]
    got, stats = _check([rows], 0, [(0, 90, 30, 2)])
    assert got[0] == (0, 5000 * 600000, main.encode()) and got[0][1] > 2 ** 31
    assert stats['pairs'] == 5002 and stats['entries'] == 3 and stats['tied_at_cut'] == 0


def test_cut_inside_a_tie_of_singletons():
    rng = random.Random(4)
    prefix = _seq(rng, 2000)
    tails = set()
    while len(tails) < 3000:
        tails.add(_seq(rng, 12))
    rows = [_row(prefix + t) for t in sorted(tails, key=lambda t: rng.random())]
    got, stats = _check([rows], 0, [(0, 2012, 100, 5)])
    assert [n for _, n, _ in got] == [1] * 5
    assert [s[2000:].decode() for _, _, s in got] == sorted(tails, reverse=True)[:5]
    assert stats['entries'] == 3000 and stats['tied_at_cut'] == 3000
    assert stats['text_bytes'] == 5 * 2012


@pytest.mark.parametrize('cut', [0, 1, 100])
def test_cut_sizes(cut):
    rows = _family(random.Random(11), n_rows=30, length=400)
    got, stats = _check([rows], 0, [(0, 300, 40, cut)])
    distinct = len(vc.expected_variants(rows, 0, 300, 40, 10 ** 6))
    assert 1 < distinct < 100 and len(got) == min(cut, distinct)
    if cut == 0:
        assert stats['pairs'] == 0 and stats['ms'] == 0       # no device work


def test_three_overlapping_regions_in_one_call():
    rows = _family(random.Random(12), n_rows=200, length=900)
    regions = [(0, 300, 50, 4), (150, 600, 100, 6), (299, 901, 80, 3)]
    got, _ = _check([rows], 0, regions)
    assert {k for k, _, _ in got} == {0, 1, 2}


def test_second_group_of_a_slot():
    first = _family(random.Random(13), n_rows=70, length=500)
    second = _family(random.Random(14), n_rows=45, length=500)
    regions = [(20, 260, 30, 8)]
    got, _ = _check([first, second], 1, regions)
    assert got and got != _want(first, regions)


def test_bad_arguments():
    ctx = session.context()
    ctx.a2c_load_rows(SLOT, ['ACGT'], [0], [1], [0, 1], a2c._CODON_CHARS)
    for args, bits in ((([-1], [4], [0], [1]), 64), (([0], [-4], [0], [1]), 64), (([], [], [], []), 64),
                       (([0], [4], [0], [1]), 7), (([0], [4], [0], [1]), 65)):
        with pytest.raises(_native.NativeError, match=r'\(-3\)'):
            ctx.a2c_variants(SLOT, 0, *args, key_bits=bits)
    with pytest.raises(_native.NativeError, match='no group'):
        ctx.a2c_variants(SLOT, 1, [0], [4], [0], [1])


# ---------------------------------------------------------------------------
# 3. a random case, 4. the collision path
# ---------------------------------------------------------------------------
RANDOM_REGIONS = [(0, 120, 30, 5), (60, 240, 40, 60), (150, 300, 20, 40)]   # seed 21: a tie at 60


def _random_rows(seed=21, n=4000):
    rng = random.Random(seed)
    base = _seq(rng, 300)
    rows = []
    for _ in range(n):
        off = rng.choice([0, 0, 3, 10, 70, 120])
        s = list(base[off:rng.choice([300, 300, 250, 200, 130])])
        for _ in range(rng.choice([0, 0, 0, 1, 1, 2])):
            s[rng.randrange(len(s))] = rng.choice('ACGTN-n')
        rows.append(_row(''.join(s), off, rng.randint(1, 5)))
    return rows


def test_random_rows():
    rows = _random_rows()
    want = _want(rows, RANDOM_REGIONS)
    assert {k for k, _, _ in want} == {0, 1, 2}
    assert any(vc.tie_at_cut(rows, *region) for region in RANDOM_REGIONS)
    got, stats = _check([rows], 0, RANDOM_REGIONS)
    assert stats['tied_at_cut'] > 0 and stats['entries'] > 100


def test_short_key_reports_a_collision():
    with pytest.raises(_native.NativeError, match='collision'):
        _device([_random_rows()], 0, RANDOM_REGIONS, key_bits=8)


# ---------------------------------------------------------------------------
# 5. the drop-in
# ---------------------------------------------------------------------------
def _small_config():
    config = vc.SCRIPTS['SequenceReportTest.testVariantReport']['calls'][3]['config']
    config = json.loads(json.dumps(config))
    assert set(config['projects']) == {'R1', 'R2', 'R3', 'R4'}
    for project in config['projects'].values():
        project['max_variants'] = 3
    return config


def _small_aligned():
    """Two seeds at two cutoffs; ties in count at and above the cut."""
    reads = {'R1-seed': [('AAATTTCGA', 0, 10), ('GGGTTTCGA', 0, 6), ('AAATTTGGG', 0, 6),
                         ('AAATTTTCA', 0, 6), ('TTTCGA', 3, 2), ('AAATTTCGATCA', 0, 1)],
             'R2-seed': [('AAATTTGGCCCGAGA', 0, 9), ('AAATTTGGCCCGAGG', 0, 9), ('AAATTTGGACCGAGA', 0, 4),
                         ('TTTGGCCCGAGA', 3, 4), ('AAATTTGGCCCG', 0, 4)]}
    lines = ['refname,qcut,rank,count,offset,seq']
    for seed, rows in reads.items():
        for qcut in ('15', '20'):
            for rank, (seq, off, count) in enumerate(rows[:len(rows) - (qcut == '20')]):
                lines.append('{},{},{},{},{},{}'.format(seed, qcut, rank, count + (qcut == '20'), off, seq))
    return '\n'.join(lines) + '\n'


def _restated_file(text, config):
    """The variants file by the oracle's coordinate mapping and the
    restatement, run by run."""
    import csv
    import itertools
    out = io.StringIO()
    a2c.SequenceReport(None, None, []).write_nuc_variants_header(out)
    rows = csv.DictReader(io.StringIO(text))
    for _, grp in itertools.groupby(rows, lambda r: (r['refname'], r['qcut'])):
        grp = list(grp)
        report = og.Report(og.Inserts(io.StringIO()), og.Projects(config), [])
        report.read(grp)
        vc.oracle_write(report, out, grp, config)
    return out.getvalue()


def _dropin(text, json_path, variants):
    outs = {k: io.StringIO() for k in OUTS}
    kwargs = dict(variants_csv=io.StringIO()) if variants else {}
    a2c.aln2counts(io.StringIO(text), outs['nuc'], outs['amino'], outs['coord_ins'], outs['conseq'],
                   failed_align_csv=outs['failed'], coverage_summary_csv=outs['coverage'],
                   json=json_path, **kwargs)
    got = {k: v.getvalue() for k, v in outs.items()}
    return got, (kwargs['variants_csv'].getvalue() if variants else None)


def test_dropin_writes_the_variants_file(tmp_path):
    config, text = _small_config(), _small_aligned()
    path = str(tmp_path / 'projects.json')
    with open(path, 'w') as f:
        json.dump(config, f)
    plain, _ = _dropin(text, path, False)
    got, variants = _dropin(text, path, True)
    want = _restated_file(text, config)
    assert want.count('\n') == 1 + 4 * 3
    assert variants == want
    assert got == plain and plain['nuc'].count('\n') > 1


# ---------------------------------------------------------------------------
# 6. the resident chain
# ---------------------------------------------------------------------------
def _pol_projects(tmp_path):
    """The default regions with a variants table of their own."""
    with open(projects.DEFAULT_PATH) as f:
        cfg = json.load(f)
    cfg['max_variants'] = {name: 4 for name in cfg['project_regions']}
    path = str(tmp_path / 'regions.json')
    with open(path, 'w') as f:
        json.dump(cfg, f)
    return path


def test_chain_variants_from_the_device_rows_and_from_the_file(tmp_path, monkeypatch):
    d = os.path.join(HERE, 'golden', 'e2e', 'syn_pol')
    r1, r2 = os.path.join(d, 'R1.fastq.gz'), os.path.join(d, 'R2.fastq.gz')
    prelim, remap_csv, aligned = (tmp_path / n for n in ('prelim.csv', 'remap.csv', 'aligned.csv'))
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    with open(prelim) as f, open(remap_csv, 'w') as out, open(tmp_path / 'counts.csv', 'w') as cn:
        rm.remap(r1, r2, f, out, cn, gzip=True, work_path=str(tmp_path))
    with open(remap_csv) as f, open(aligned, 'w') as out:
        s2a.sam2aln(f, out)
    proj = _pol_projects(tmp_path)

    def run(tag):
        paths = {k: tmp_path / '{}_{}.csv'.format(tag, k) for k in OUTS + ('variants',)}
        hs = {k: open(p, 'w') for k, p in paths.items()}
        try:
            with open(aligned) as f:
                a2c.aln2counts(f, hs['nuc'], hs['amino'], hs['coord_ins'], hs['conseq'],
                               failed_align_csv=hs['failed'], coverage_summary_csv=hs['coverage'],
                               json=proj, variants_csv=hs['variants'])
        finally:
            for h in hs.values():
                h.close()
        return {k: p.read_text() for k, p in paths.items()}
    dev = run('dev')
    assert session.stats['aln2counts_source'] == 'device'
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    csv_way = run('csv')
    assert session.stats['aln2counts_source'] == 'csv'
    assert dev['variants'] == csv_way['variants']
    assert dev['variants'].count('\n') > 4
    assert dev == csv_way
    with gzip.open(os.path.join(d, 'a2c_nuc.csv.gz'), 'rt') as f:
        assert dev['nuc'] == f.read()


# ---------------------------------------------------------------------------
# 7. two ranks
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_two_ranks_take_the_unsplit_path(tmp_path):
    d = str(tmp_path)
    with open(os.path.join(d, 'aligned.csv'), 'w') as f:
        f.write(_small_aligned())
    with open(os.path.join(d, 'projects.json'), 'w') as f:
        json.dump(_small_config(), f)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE='2',
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, WORKER, '--dir', d],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    for k in OUTS + ('variants',):
        got = open(os.path.join(d, k + '.csv')).read()
        assert got == open(os.path.join(d, k + '.single')).read(), k
    assert open(os.path.join(d, 'variants.csv')).read() == _restated_file(_small_aligned(), _small_config())
    stats = [json.load(open(os.path.join(d, 'rank%d.json' % r))) for r in range(2)]
    assert [s.get('mode') for s in stats] == ['unsplit', 'unsplit'], stats

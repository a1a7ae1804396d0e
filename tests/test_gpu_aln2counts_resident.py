"""aln2counts() from the resident sam2aln pass (mh_a2c_load_resident,
k_a2c_stage, k_a2c_bin_count / _scan / _fill): when aligned.csv is the
unchanged file this process's sam2aln() just wrote, its rows, codon extents
and bin lists are built on the device from what sam2aln left there instead
of parsed from the file.  Every report must be the bytes the file path
writes (the goldens are the reference's own outputs), the device table must
equal the one mh_a2c_load_csv builds from the same text, and every other
input must go through the file path as before."""
import gzip
import io
import os
import shutil

import numpy as np
import pytest

from micall_amd import _native, projects, session
from micall_amd import aln2counts as a2c
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
CASES = sorted(os.listdir(E2E_DIR))
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'failed', 'coverage')
HEADER = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'
CODONS = a2c._CODON_CHARS


def _golden(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.gz'), 'rt') as f:
        return f.read()


def _chain_to_aligned(case, tmp_path):
    """prelim_map, remap and sam2aln on files, as bin/micall chains them."""
    r1 = os.path.join(E2E_DIR, case, 'R1.fastq.gz')
    r2 = os.path.join(E2E_DIR, case, 'R2.fastq.gz')
    r2 = r2 if os.path.exists(r2) else None
    prelim, remap_csv, aligned = (tmp_path / n for n in ('prelim.csv', 'remap.csv', 'aligned.csv'))
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    with open(prelim) as f, open(remap_csv, 'w') as out, open(tmp_path / 'counts.csv', 'w') as cn:
        rm.remap(r1, r2, f, out, cn, gzip=True, work_path=str(tmp_path))
    with open(remap_csv) as f, open(aligned, 'w') as out:
        s2a.sam2aln(f, out)
    return aligned


def _aln2counts(handle, tmp_path, tag):
    """aln2counts() on an open aligned.csv into files; the six reports."""
    paths = {k: tmp_path / '{}_{}.csv'.format(tag, k) for k in OUTS}
    hs = {k: open(p, 'w') for k, p in paths.items()}
    try:
        a2c.aln2counts(handle, hs['nuc'], hs['amino'], hs['coord_ins'], hs['conseq'],
                       failed_align_csv=hs['failed'], coverage_summary_csv=hs['coverage'])
    finally:
        for h in hs.values():
            h.close()
    return {k: p.read_text() for k, p in paths.items()}


def _aln2counts_path(path, tmp_path, tag):
    with open(path) as f:
        got = _aln2counts(f, tmp_path, tag)
        assert f.tell() == os.path.getsize(path)      # consumed, whichever way it went
    return got


# ---------------------------------------------------------------------------
# 1. the chain on the golden cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_chain_parity_on_the_device_rows(case, tmp_path):
    """prelim_map -> remap -> sam2aln -> aln2counts in one process: every
    report is the reference's, and aln2counts took the device rows on every
    case: syn_chimera (whose remap.csv sam2aln parses) and the two cases
    without rows (0 groups) included."""
    aligned = _chain_to_aligned(case, tmp_path)
    assert aligned.read_text() == _golden(case, 'aligned.csv')
    got = _aln2counts_path(aligned, tmp_path, 'dev')
    assert session.stats['aln2counts_source'] == 'device'
    for k in OUTS:
        assert got[k] == _golden(case, 'a2c_{}.csv'.format(k)), k


@pytest.mark.parametrize('case', ['syn_pol_indel', 'micro_2100A-HCV-1337B-V3LOOP'])
def test_chain_with_the_file_path_forced(case, tmp_path, monkeypatch):
    aligned = _chain_to_aligned(case, tmp_path)
    monkeypatch.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')
    got = _aln2counts_path(aligned, tmp_path, 'csv')
    assert session.stats['aln2counts_source'] == 'csv'
    for k in OUTS:
        assert got[k] == _golden(case, 'a2c_{}.csv'.format(k)), k


# ---------------------------------------------------------------------------
# 2. the layout kernels at their edges (no mapper: a synthetic remap.csv)
# ---------------------------------------------------------------------------
OFFSETS = (0, 1, 2, 59, 60, 61, 62, 63, 64, 65, 66, 125, 126, 127, 128)   # frames; bin edges at 63, 126
LENGTHS = (1, 2, 3, 4, 61, 62, 63, 64, 65, 126, 600)
CUTS = [10, 15, 20]
Q12, Q17, Q40 = '-', '2', 'I'


def _edge_reads(seed):
    """Reads of a synthetic remap.csv: (rname, offset, seq, qual) is an
    unpaired row, a pair of them two mates.  'sweep': every offset x length;
    'rows1023' / 'rows1024' / 'rows1025': that many distinct 30-nt rows at
    one offset (the 1024-row chunk of k_a2c_count, the 256-row blocks of the
    bin kernels); 'one': a group of one row; some reads repeated, so counts
    above 1 and runs of equal counts both occur.  Only mates are merged at a
    quality cutoff (an unpaired read is taken as it is, sam2aln.py:392-395),
    so the reads whose qualities lie on both sides of the cutoffs are pairs:
    'lowq' passes only cutoff 10 and 'midq' cutoffs 10 and 15 (their other
    (rname, cutoff) groups are empty), 'mixq' passes all three with
    different Ns."""
    rng = np.random.default_rng(seed)

    def seq(n):
        return ''.join('ACGT'[k] for k in rng.integers(0, 4, size=n))

    def pair(name, off, n, qual_at):
        whole = seq(n + 20)             # the mates overlap in all but 20 bases each
        quals = ''.join(qual_at(off + i) for i in range(n + 20))
        return ((name, off, whole[:n], quals[:n]), (name, off + 20, whole[20:], quals[20:]))

    reads = [('sweep', off, seq(n), Q40 * n) for off in OFFSETS for n in LENGTHS]
    for k in range(0, 60, 4):
        reads += [reads[k]] * (1 + k % 3)
    for n in (1023, 1024, 1025):
        rows = set()
        while len(rows) < n:
            rows.add(seq(30))
        reads += [('rows%d' % n, 7, s, Q40 * 30) for s in sorted(rows)]
    reads.append(('one', 5, seq(40), Q40 * 40))
    for name, q in (('lowq', Q12), ('midq', Q17)):
        reads += [pair(name, 3 * k + k % 3, 50 + k, lambda at, q=q: q) for k in range(20)]
    reads += [pair('mixq', k, 90, lambda at: (Q12, Q17, Q40, Q40, Q40)[at % 5]) for k in range(12)]
    return [reads[i] for i in rng.permutation(len(reads))]


def _remap_text(reads):
    rows = []
    for i, read in enumerate(reads):
        mates = read if isinstance(read[0], tuple) else (read,)
        for flag, (name, off, s, q) in zip((99, 147) if len(mates) == 2 else (0,), mates):
            rows.append('r{},{},{},{},44,{}M,*,0,0,{},{}\n'.format(i, flag, name, off + 1, len(s), s, q))
    return HEADER + ''.join(rows)


def _tables_equal(ctx, a, b, n_groups, ranges):
    for g in range(n_groups):
        info = ctx.a2c_group(a, g)
        assert info == ctx.a2c_group(b, g), g
        for frame in range(3):
            got = ctx.a2c_counts(a, g, frame, info['ncod'][frame])
            want = ctx.a2c_counts(b, g, frame, info['ncod'][frame])
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (g, frame)
            for lefts, rights in ranges:
                assert (ctx.a2c_inserts(a, g, frame, lefts, rights) ==
                        ctx.a2c_inserts(b, g, frame, lefts, rights)), (g, frame, lefts)


INSIDE = ([0, 2, 21, 41], [3, 12, 30, 44])      # codon ranges inside the rows
PAST = ([1000000], [1000005])                   # and past the end of every row


def test_device_layout_equals_the_parsed_file():
    reads = _edge_reads(5)
    assert 3000 < len(reads) < 6000
    ctx = _native.Context(0)
    try:
        serial = ctx.sam2aln_serial
        ctx.sam2aln_csv(_remap_text(reads), q_cutoffs=CUTS)
        assert ctx.sam2aln_serial == serial + 1
        n = ctx.a2c_load_resident(0, CODONS)
        text = ctx.sam2aln_output('aligned')
        assert n is not None and n == ctx.a2c_load_csv(1, text, CODONS)
        groups = [ctx.a2c_group(0, g) for g in range(n)]
        keys = [(g['refname'], g['qcut']) for g in groups]
        # the shapes this test is about are all there
        sizes = {k: g['n_rows'] for k, g in zip(keys, groups)}
        for rows in (1023, 1024, 1025):
            assert [sizes[('rows%d' % rows, str(q))] for q in CUTS] == [rows] * 3
        assert sizes[('one', '15')] == 1
        assert ('lowq', '10') in sizes and ('midq', '15') in sizes and ('mixq', '20') in sizes
        assert not {('lowq', '15'), ('lowq', '20'), ('midq', '20')} & set(sizes)
        counts = [int(line.split(',')[3]) for line in text.splitlines()[1:]]
        assert max(counts) > 1 and counts.count(1) > 1000       # ties the sequence decides
        assert any(g['ncod'][0] > 2 * 21 for g in groups)       # more than two bins
        _tables_equal(ctx, 0, 1, n, (INSIDE, PAST))
        assert any(ctx.a2c_inserts(0, g, 0, *INSIDE) for g in range(n))
        assert not any(ctx.a2c_inserts(0, g, 0, *PAST) for g in range(n))
        timing = ctx.a2c_timing(0)
        assert len(timing) == 3 and timing[0] > 0 and timing[1] > 0
    finally:
        ctx.close()


def test_order_is_built_without_formatting_and_after_it():
    """The row order comes from one place: loading before aligned.csv was
    ever formatted and after give the same table, and the same text."""
    reads = _edge_reads(6)[:400]
    ctx, ctx2 = _native.Context(0), _native.Context(0)
    try:
        ctx.sam2aln_csv(_remap_text(reads), q_cutoffs=CUTS)
        ctx2.sam2aln_csv(_remap_text(reads), q_cutoffs=CUTS)
        n = ctx.a2c_load_resident(0, CODONS)          # nothing formatted yet
        text = ctx2.sam2aln_output('aligned')
        assert ctx2.a2c_load_resident(0, CODONS) == n           # formatted before
        assert ctx.sam2aln_output('aligned') == text
        assert ctx.a2c_load_csv(1, text, CODONS) == n
        _tables_equal(ctx, 0, 1, n, (INSIDE,))
        info = [ctx.a2c_group(0, g) for g in range(n)]
        assert info == [ctx2.a2c_group(0, g) for g in range(n)]
    finally:
        ctx.close()
        ctx2.close()


# ---------------------------------------------------------------------------
# 3. fallbacks
# ---------------------------------------------------------------------------
def test_no_sam2aln_result_in_the_context():
    ctx = _native.Context(0)
    try:
        assert ctx.a2c_load_resident(0, CODONS) is None         # no call yet
        ctx.sam2aln_csv(_remap_text(_edge_reads(7)[:50]), q_cutoffs=[15])
        assert ctx.a2c_load_resident(0, CODONS) is not None
        with pytest.raises(_native.NativeError):                # a call that fails
            ctx.sam2aln_csv(HEADER + 'r0,0,ref,1,44,5M,*,0,0,ACGTACGTAC,IIIIIIIIII\n', q_cutoffs=[15])
        assert ctx.a2c_load_resident(0, CODONS) is None
        # a reference name the file would quote
        unpaired = [r for r in _edge_reads(7)[:60] if not isinstance(r[0], tuple)]
        reads = [('"ref,a"' if k % 2 else 'ref', off, s, q) for k, (_name, off, s, q) in enumerate(unpaired)]
        ctx.sam2aln_csv(_remap_text(reads), q_cutoffs=[15])
        assert ctx.sam2aln_output('aligned').count('"ref,a",15,') > 5
        assert ctx.a2c_load_resident(0, CODONS) is None
    finally:
        ctx.close()


SEEDS = ('HIV1B-pol-seed', 'ERCC-00002-seed')     # references aln2counts() knows


def _sample_reads(seed, n=300):
    """(rname, offset, seq, qual) of unpaired reads cut from two seed
    references with a few substitutions, at mixed qualities."""
    rng = np.random.default_rng(seed)
    refs = projects.load_default().seed_sequences()
    reads = []
    for k in range(n):
        name = SEEDS[k % 3 == 0]
        ref = refs[name]
        off = int(rng.integers(0, 600))
        s = list(ref[off:off + int(rng.integers(40, 260))])
        for at in rng.integers(0, len(s), size=2):
            s[at] = 'ACGT'[int(rng.integers(0, 4))]
        qual = ''.join((Q40, Q40, Q17, Q12)[int(x)] for x in rng.integers(0, 4, size=len(s)))
        reads.append((name, off, ''.join(s), Q40 * len(s) if k % 2 else qual))
    return reads + reads[:n // 10]          # some sequences seen twice


def _sam2aln_to_file(remap_text, tmp_path, name='aligned.csv', **kw):
    """sam2aln() from a remap.csv file into an aligned.csv file."""
    remap_csv = tmp_path / ('remap_' + name)
    remap_csv.write_text(remap_text)
    aligned = tmp_path / name
    with open(remap_csv) as f, open(aligned, 'w') as out:
        s2a.sam2aln(f, out, **kw)
    return aligned


def _outcome(run):
    """What a run gave, or the text of what it raised."""
    try:
        return run()
    except Exception as e:
        return '{}: {}'.format(type(e).__name__, e)


def _file_path_outcome(path, tmp_path, monkeypatch, prepare=None):
    """The file path's own outcome on `path` (the resident path switched off)."""
    with monkeypatch.context() as m:
        m.setenv('MICALL_ALN2COUNTS_RESIDENT', '0')

        def run():
            with open(path) as f:
                if prepare:
                    prepare(f)
                return _aln2counts(f, tmp_path, 'want')
        want = _outcome(run)
        assert session.stats['aln2counts_source'] == 'csv'
    return want


def test_written_file_takes_the_device_rows(tmp_path, monkeypatch):
    """The control of the fallbacks below: the same sample, left alone."""
    aligned = _sam2aln_to_file(_remap_text(_sample_reads(8)), tmp_path, q_cutoffs=CUTS)
    got = _aln2counts_path(aligned, tmp_path, 'got')
    assert session.stats['aln2counts_source'] == 'device'
    assert got == _file_path_outcome(aligned, tmp_path, monkeypatch)
    assert got['nuc'].count('\n') > 1


@pytest.mark.parametrize('kind', ['edited', 'truncated', 'other_sample', 'copy', 'comma_in_rname'])
def test_fallbacks_parse_the_file(kind, tmp_path, monkeypatch):
    reads = _sample_reads(8)
    if kind == 'comma_in_rname':
        reads = [('"ref,a"' if name == SEEDS[1] else name, off, s, q) for name, off, s, q in reads]
    aligned = _sam2aln_to_file(_remap_text(reads), tmp_path, q_cutoffs=CUTS)
    path = aligned
    if kind == 'edited':            # the same size, another base
        data = aligned.read_bytes()
        at = data.rindex(b'A')
        aligned.write_bytes(data[:at] + b'C' + data[at + 1:])
    elif kind == 'truncated':
        data = aligned.read_bytes()
        aligned.write_bytes(data[:data.rindex(b'\n', 0, len(data) - 1) + 1])
    elif kind == 'other_sample':    # sam2aln() again, on another input, before aln2counts()
        _sam2aln_to_file(_remap_text(_sample_reads(9)), tmp_path, 'other.csv', q_cutoffs=CUTS)
    elif kind == 'copy':
        path = tmp_path / 'copy.csv'
        shutil.copyfile(aligned, path)
    else:
        assert '"ref,a",10,' in aligned.read_text()
    got = _outcome(lambda: _aln2counts_path(path, tmp_path, 'got'))
    assert session.stats['aln2counts_source'] == 'csv'
    if kind == 'comma_in_rname':    # no such seed: both ways end in the same KeyError
        assert got.startswith('KeyError')
    else:
        assert isinstance(got, dict) and got['nuc'].count('\n') > 1
    assert got == _file_path_outcome(path, tmp_path, monkeypatch)


def test_handle_read_past_its_start_is_not_the_file(tmp_path, monkeypatch):
    aligned = _sam2aln_to_file(_remap_text(_sample_reads(8)), tmp_path, q_cutoffs=CUTS)

    def run():
        with open(aligned) as f:
            f.readline()
            return _aln2counts(f, tmp_path, 'got')
    got = _outcome(run)
    assert session.stats['aln2counts_source'] == 'csv'
    assert got == _file_path_outcome(aligned, tmp_path, monkeypatch, prepare=lambda f: f.readline())


def test_seq_character_outside_the_alphabet_raises_the_file_paths_error(tmp_path, monkeypatch):
    """An 'R' in a SEQ reaches aligned.csv; the device finds it (class
    A2C_BAD) and the file path then names row and character as ever.  The
    library's message is also the one a StringIO of the file gets; only the
    entry point the binding names in front of it differs between a file
    (mh_a2c_load_file) and a text (mh_a2c_load_csv), as it always has."""
    reads = _sample_reads(8)
    name, off, s, q = reads[17]
    reads[17] = (name, off, s[:len(s) // 2] + 'R' + s[len(s) // 2 + 1:] if len(s) > 1 else 'R', q)
    aligned = _sam2aln_to_file(_remap_text(reads), tmp_path, q_cutoffs=[15])
    assert 'R' in aligned.read_text().split('\n', 1)[1]
    got = _outcome(lambda: _aln2counts_path(aligned, tmp_path, 'got'))
    assert session.stats['aln2counts_source'] == 'csv'
    assert got.startswith('NativeError: ') and "character 'R'" in got
    assert got == _file_path_outcome(aligned, tmp_path, monkeypatch)
    text = _outcome(lambda: _aln2counts(io.StringIO(aligned.read_text()), tmp_path, 'text'))
    assert text.startswith('NativeError: ')
    assert got.split('): ', 1)[1] == text.split('): ', 1)[1]


# ---------------------------------------------------------------------------
# 4. the slot owns its bytes
# ---------------------------------------------------------------------------
def test_slot_survives_the_next_sam2aln(tmp_path):
    first = _sample_reads(10)
    aligned = _sam2aln_to_file(_remap_text(first), tmp_path, q_cutoffs=[15])
    _aln2counts_path(aligned, tmp_path, 'got')
    assert session.stats['aln2counts_source'] == 'device'
    ctx = session.context()
    slot = a2c.SLOT_REPORT
    n = ctx.a2c_load_csv(2, aligned.read_text(), CODONS)
    groups = [ctx.a2c_group(slot, g) for g in range(n)]
    assert groups == [ctx.a2c_group(2, g) for g in range(n)]
    before = [ctx.a2c_inserts(slot, g, 0, *INSIDE) for g in range(n)]
    assert any(before)
    # another, larger sample through the same sam2aln state
    _sam2aln_to_file(_remap_text(_sample_reads(11, 2000)), tmp_path, 'second.csv', q_cutoffs=CUTS)
    after = [ctx.a2c_inserts(slot, g, 0, *INSIDE) for g in range(n)]
    assert after == before
    assert after == [ctx.a2c_inserts(2, g, 0, *INSIDE) for g in range(n)]

"""sam2aln() from the resident remap pass (mh_sam2aln_resident, k_s2a_stage):
when remap.csv is the unchanged file this process's remap() just wrote, the
rows are built on the device from the resident reads and records instead of
parsed from the file.  The three outputs must be the bytes the file path
writes (the goldens are the reference's own outputs on the same remap.csv),
and every other input must go through the file path as before."""
import csv
import gzip
import io
import os
import re

import numpy as np
import pytest

import og_sam2aln
from micall_amd import _native, projects, session, synth
from micall_amd import prelim_map as pm
from micall_amd import remap as rm
from micall_amd import sam2aln as s2a

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E2E_DIR = os.path.join(HERE, 'golden', 'e2e')
CASES = sorted(os.listdir(E2E_DIR))
OUTPUTS = ('aligned.csv', 'insert.csv', 'failed.csv')
HEADER = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'


def _golden(case, name):
    with gzip.open(os.path.join(E2E_DIR, case, name + '.gz'), 'rt') as f:
        return f.read()


def _inputs(case):
    r1 = os.path.join(E2E_DIR, case, 'R1.fastq.gz')
    r2 = os.path.join(E2E_DIR, case, 'R2.fastq.gz')
    return r1, (r2 if os.path.exists(r2) else None)


def _fastq_qnames(path, paired):
    """bowtie2's QNAME of every record: the header up to the first
    whitespace, a trailing /1 or /2 dropped for mates."""
    out = []
    with gzip.open(path, 'rt') as f:
        for k, line in enumerate(f):
            if k % 4 == 0:
                name = line[1:].split()[0] if line[1:].split() else ''
                if paired:
                    name = re.sub(r'/[12]$', '', name)
                out.append(name)
    return out


def _expected_source(case):
    """'device' exactly when the golden remap.csv holds one row per FASTQ
    read in FASTQ order (mates interleaved): computed from the goldens."""
    r1, r2 = _inputs(case)
    n1 = _fastq_qnames(r1, r2 is not None)
    if r2 is None:
        reads = n1
    else:
        n2 = _fastq_qnames(r2, True)
        reads = [n for pair in zip(n1, n2) for n in pair]
    rows = [row[0] for row in csv.reader(io.StringIO(_golden(case, 'remap.csv')))][1:]
    return 'device' if rows and rows == reads else 'csv'


def _chain_to_remap(case, tmp_path):
    """prelim_map to a file, remap to files, as bin/micall chains them."""
    r1, r2 = _inputs(case)
    prelim = tmp_path / 'prelim.csv'
    with open(prelim, 'w') as f:
        pm.prelim_map(r1, r2, f, gzip=True)
    remap_csv = tmp_path / 'remap.csv'
    with open(prelim) as f, open(remap_csv, 'w') as out, open(tmp_path / 'counts.csv', 'w') as cn:
        rm.remap(r1, r2, f, out, cn, gzip=True, work_path=str(tmp_path))
    return remap_csv


def _sam2aln_files(remap_handle, tmp_path, tag, **kw):
    paths = [tmp_path / '{}_{}'.format(tag, n) for n in OUTPUTS]
    handles = [open(p, 'w') for p in paths]
    try:
        s2a.sam2aln(remap_handle, *handles, **kw)
    finally:
        for h in handles:
            h.close()
    return tuple(p.read_text() for p in paths)


def _golden_outputs(case):
    return tuple(_golden(case, n) for n in OUTPUTS)


SOURCES_SEEN = {}


@pytest.mark.parametrize('case', CASES)
def test_chain_parity_and_source(case, tmp_path):
    """prelim_map -> remap -> sam2aln in one process on every golden case:
    the outputs are the reference's whichever way sam2aln took, and it took
    the device rows exactly when remap.csv is one row per read in order."""
    remap_csv = _chain_to_remap(case, tmp_path)
    assert remap_csv.read_text() == _golden(case, 'remap.csv')
    with open(remap_csv) as f:
        got = _sam2aln_files(f, tmp_path, 'out')
        assert f.tell() == os.path.getsize(remap_csv)      # consumed, as the reference leaves it
    assert got == _golden_outputs(case)
    want = _expected_source(case)
    SOURCES_SEEN[case] = session.stats['sam2aln_source']
    assert session.stats['sam2aln_source'] == want


def test_most_cases_take_the_device_rows(tmp_path_factory):
    """The parity test above must have exercised the new path: at least 15
    of the 20 golden cases qualify (17 do: all but syn_chimera, whose split
    pairs are mapped again and appended, and the two cases without rows)."""
    for case in CASES:
        if case not in SOURCES_SEEN:        # this test run on its own
            d = tmp_path_factory.mktemp('chain')
            with open(_chain_to_remap(case, d)) as f:
                _sam2aln_files(f, d, 'out')
            SOURCES_SEEN[case] = session.stats['sam2aln_source']
    assert sum(1 for v in SOURCES_SEEN.values() if v == 'device') >= 15, SOURCES_SEEN


# ---------------------------------------------------------------------------
# the stage kernel: staged rows == printed rows
# ---------------------------------------------------------------------------
TRIMS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 251, 300, 301, 600)


def _synthetic_reads(n_pairs=2000):
    pol = projects.load_default().seed_sequences()['HIV1B-pol-seed']
    pairs = synth.make_pairs(n_pairs, genomes={'HIV1B-pol-seed': pol}, genome_seed=31, read_seed=32,
                             read_len=600, indel_rate=0.01, err_rate=0.01)
    names, seqs, quals = synth.interleave(pairs)
    names = [n[1:].split()[0] for n in names]
    rng = np.random.default_rng(33)
    out_s, out_q = [], []
    for r, (s, q) in enumerate(zip(seqs, quals)):
        # long reads dominate so that the long reverse-strand case is well
        # covered; every trim length appears on both mates (17 is odd)
        L = TRIMS[r % len(TRIMS)] if r % 3 == 0 else (600, 301, 300, 251)[r % 4]
        s, q = list(s[:L]), q[:L]
        if r % 5 == 0:
            for at in (0, L - 1, 15, 31):
                if 0 <= at < L and rng.random() < 0.7:
                    s[at] = 'N'
        out_s.append(''.join(s))
        out_q.append(q)
    # some pairs of noise: both mates unmapped at full length
    for p in range(0, n_pairs, 50):
        for m in (0, 1):
            L = len(out_s[2 * p + m])
            out_s[2 * p + m] = ''.join('ACGT'[k] for k in rng.integers(0, 4, size=L))
    return pol, names, out_s, out_q


def test_staged_rows_equal_printed_rows():
    pol, names, seqs, quals = _synthetic_reads()
    n = len(seqs)
    ctx, ctx2 = _native.Context(0), _native.Context(0)
    try:
        ctx.index_build(['HIV1B-pol-seed'], [pol], 20)
        ctx.reads_load(seqs, quals, True, names=names)
        ctx.map(_native.params(_native.LOCAL))
        # coverage, from the records themselves
        rec = ctx.rec_fields(('ref', 'pos', 'rev'))
        lens = np.array([len(s) for s in seqs])
        mapped, rev = rec[:, 0] >= 0, rec[:, 2] != 0
        assert int((mapped & rev & (lens > 256)).sum()) >= 200
        assert int((mapped & ~rev & (lens > 256)).sum()) >= 200
        assert int((~mapped[0::2] & ~mapped[1::2]).sum()) >= 20
        assert int((~mapped & (lens < 16)).sum()) >= 10
        for at in (0, 15, 31):
            assert sum(1 for s, m in zip(seqs, mapped) if m and len(s) > 256 and s[at] == 'N') >= 10
        assert sum(1 for s, m in zip(seqs, mapped) if m and len(s) > 256 and s[-1] == 'N') >= 10

        units = ctx.sam2aln_resident(['HIV1B-pol-seed'], q_cutoffs=[15])
        assert units == n // 2
        got_len, got_seq, got_qual = ctx.sam2aln_resident_rows()
        rows_text = ctx.format_rows(1, 0, n)
        rows = list(csv.reader(io.StringIO(rows_text)))
        assert len(rows) == n
        at = 0
        for r, row in enumerate(rows):
            L = int(got_len[r])
            assert L == len(seqs[r])
            assert got_seq[at:at + L].decode() == row[9], (r, len(seqs[r]), row[1])
            assert got_qual[at:at + L].decode() == row[10], (r, len(seqs[r]), row[1])
            at += L
        assert at == len(got_seq) == len(got_qual)

        ctx2.sam2aln_csv(HEADER + rows_text)
        for which in ('aligned', 'insert', 'failed'):
            assert ctx.sam2aln_output(which) == ctx2.sam2aln_output(which), which
        assert ctx.sam2aln_stats() == ctx2.sam2aln_stats()
        assert ctx.sam2aln_output('insert').count('\n') > 1     # insertions were covered
    finally:
        ctx.close()
        ctx2.close()


def test_resident_needs_a_mapping_pass_and_names():
    pol = projects.load_default().seed_sequences()['HIV1B-pol-seed']
    ctx = _native.Context(0)
    try:
        ctx.index_build(['HIV1B-pol-seed'], [pol], 20)
        ctx.reads_load([pol[:100], pol[200:300]], ['I' * 100] * 2, True)
        with pytest.raises(_native.NativeError):
            ctx.sam2aln_resident(['HIV1B-pol-seed'])             # no mapping pass
        ctx.map(_native.params(_native.LOCAL))
        with pytest.raises(_native.NativeError):
            ctx.sam2aln_resident(['HIV1B-pol-seed'])             # no names
        with pytest.raises(_native.NativeError):
            ctx.sam2aln_resident_rows()                          # nothing staged
    finally:
        ctx.close()


def test_names_that_pair_otherwise_go_to_the_file():
    """Mates with two QNAMEs, or unpaired reads sharing one, pair in
    matchmaker otherwise than the reads do: the resident call declines."""
    pol = projects.load_default().seed_sequences()['HIV1B-pol-seed']
    ctx = _native.Context(0)
    try:
        ctx.index_build(['HIV1B-pol-seed'], [pol], 20)
        seqs, quals = [pol[:100], pol[200:300]], ['I' * 100] * 2
        for paired, names, ok in ((True, ['a', 'a'], True), (True, ['a', 'b'], False),
                                  (False, ['a', 'b'], True), (False, ['a', 'a'], False)):
            ctx.reads_load(seqs, quals, paired, names=names)
            ctx.map(_native.params(_native.LOCAL))
            got = ctx.sam2aln_resident(['HIV1B-pol-seed'])
            assert (got is not None) == ok, (paired, names)
            if ok:
                text = HEADER + ctx.format_rows(1, 0, 2)
                assert (ctx.sam2aln_output('aligned'), ctx.sam2aln_output('insert'),
                        ctx.sam2aln_output('failed')) == og_sam2aln.sam2aln(text)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# several cutoffs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['syn_pol_indel', 'syn_maxremaps'])
def test_several_cutoffs_equal_the_file_path(case, tmp_path, monkeypatch):
    cuts = [0, 15, 30, 93]
    remap_csv = _chain_to_remap(case, tmp_path)
    with open(remap_csv) as f:
        dev = _sam2aln_files(f, tmp_path, 'dev', q_cutoffs=cuts)
    assert session.stats['sam2aln_source'] == 'device'
    monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    with open(remap_csv) as f:
        ref = _sam2aln_files(f, tmp_path, 'ref', q_cutoffs=cuts)
    assert session.stats['sam2aln_source'] == 'csv'
    assert dev == ref
    assert dev[0].count('\n') > 4


# ---------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------
CASE = 'syn_pol_indel'


def test_unchanged_file_stays_on_the_device(tmp_path):
    """A second call on a fresh handle, and the same bytes written again to
    the same file (the crc32 rule), still take the device rows."""
    remap_csv = _chain_to_remap(CASE, tmp_path)
    for step in ('first', 'second', 'rewritten'):
        if step == 'rewritten':
            remap_csv.write_bytes(remap_csv.read_bytes())
        with open(remap_csv) as f:
            got = _sam2aln_files(f, tmp_path, step)
        assert session.stats['sam2aln_source'] == 'device', step
        assert got == _golden_outputs(CASE), step


def _drop_one_pair(data):
    lines = data.split(b'\n')
    return b'\n'.join(lines[:7] + lines[9:])      # header + 6 rows kept, rows 7 and 8 (one pair) dropped


@pytest.mark.parametrize('kind', ['crlf', 'pair_removed', 'stringio', 'other_sample', 'env'])
def test_fallbacks_parse_the_file(kind, tmp_path, monkeypatch):
    remap_csv = _chain_to_remap(CASE, tmp_path)
    want = _golden_outputs(CASE)
    if kind == 'crlf':
        remap_csv.write_bytes(remap_csv.read_bytes().replace(b'\n', b'\r\n'))
    elif kind == 'pair_removed':
        data = _drop_one_pair(remap_csv.read_bytes())
        remap_csv.write_bytes(data)
        rows = list(csv.reader(io.StringIO(data.decode())))
        assert rows[6][0] != rows[7][0] and rows[7][0] == rows[8][0]    # whole pairs remain
        want = og_sam2aln.sam2aln(data.decode())
        assert want != _golden_outputs(CASE)
    elif kind == 'other_sample':
        r1, r2 = _inputs('micro_2000A-V3LOOP')
        pm.prelim_map(r1, r2, io.StringIO(), gzip=True)
    elif kind == 'env':
        monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    if kind == 'stringio':
        got = _sam2aln_files(io.StringIO(remap_csv.read_text()), tmp_path, 'out')
    else:
        with open(remap_csv) as f:
            got = _sam2aln_files(f, tmp_path, 'out')
    assert session.stats['sam2aln_source'] == 'csv'
    assert got == want


def test_handle_read_past_its_start_is_not_the_file(tmp_path, monkeypatch):
    """A handle something has read from already is handed to the file path,
    which sees what is left of it, exactly as without the resident rows."""
    remap_csv = _chain_to_remap(CASE, tmp_path)

    def run(tag):
        with open(remap_csv) as f:
            f.readline()
            try:
                return _sam2aln_files(f, tmp_path, tag)
            except Exception as e:      # the header row is gone: the parser may refuse the rest
                return type(e)

    got = run('dev')
    assert session.stats['sam2aln_source'] == 'csv'
    monkeypatch.setenv('MICALL_SAM2ALN_RESIDENT', '0')
    assert run('ref') == got

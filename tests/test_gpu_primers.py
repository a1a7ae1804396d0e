"""Anchored 5' primer trimming on the device (micall_amd.trim_fastqs, k_primer
in csrc/mh_censor.hip) against tests/primer_oracle.py applied to what
oracle/og_censor.py (and tests/trim_oracle.py, with adapters) makes of the
same file: the literal cases, directed records, one fuzz file through every
path of the drop-in, bad cycles first, adapters and primers in one call, a
read past the adapters' cap, the primers cleared after the call, the
library's refusals, the command line, and the writer unchanged without
primers."""
import csv
import gzip
import io
import json
import os

import pytest

import primer_cases
import primer_oracle
import trim_cases
from micall_amd import _native, censor_fastq, session, trim_fastqs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
P, E = primer_cases.P, primer_cases.E


def _trim_bytes(data, primers, adapters=((), None), use_gzip=False, **kwargs):
    dest, summary, primer_summary = io.BytesIO(), io.StringIO(), io.StringIO()
    result = trim_fastqs.trim(io.BytesIO(gzip.compress(data, 1) if use_gzip else data), dest, adapters[0],
                              adapters[1], use_gzip=use_gzip, summary_file=summary, primers1=primers[0],
                              primers2=primers[1], primer_summary_file=primer_summary, **kwargs)
    out = dest.getvalue()
    return (gzip.decompress(out) if use_gzip else out), result, summary.getvalue(), primer_summary.getvalue()


def _summary(n, total):
    return 'avg_quality,base_count\n{},{}\n'.format(repr(total / n), n)


def test_literals():
    """The values the rules were checked on, on the device: a 22-base primer
    at rate 0.1 in front of a 70-base insert."""
    data = primer_cases.literals_fastq()
    got, result, _, primer_summary = _trim_bytes(data, ([P], None))
    lines, src = got.split(b'\n'), data.split(b'\n')
    for i, (name, read, lead, _) in enumerate(primer_cases.LITERALS):
        assert lines[4 * i + 1].decode() == read[lead or 0:], name
        assert lines[4 * i + 3] == src[4 * i + 3][lead or 0:], name
        assert lines[4 * i] == src[4 * i] and lines[4 * i + 2] == b'+'
    want, stats = primer_oracle.trim_bytes(data, [P], [P], E)
    assert got == want and primer_cases.stats_of(result) == stats
    leads = [lead for _, _, lead, _ in primer_cases.LITERALS]
    assert result['primer_reads'] == sum(x is not None for x in leads)
    assert result['primer_bases'] == sum(x or 0 for x in leads)
    assert result['reads'] == result['bases'] == 0 and result['adapters'] == []
    rows = list(csv.DictReader(io.StringIO(primer_summary)))
    assert rows == [dict(direction=str(d), name='primer1', primer=P, reads=str(stats[(d, 0)][0]),
                         bases=str(stats[(d, 0)][1])) for d in (1, 2)]
    # the longer of two matching primers wins, of two equal ones the first
    one = primer_cases.record(0, 1, P + primer_cases.INSERT).encode()
    assert primer_cases.stats_of(_trim_bytes(one, ([P[:12], P], None))[1]) == {(1, 1): [1, 22]}
    assert primer_cases.stats_of(_trim_bytes(one, ({'a': P, 'b': P}, None))[1]) == {(1, 0): [1, 22]}


def test_directed_records():
    """Primers of 8 and 64 bases, a lead of 70, reads of 0, 7, 8, m - E - 1,
    m - E, 69, 70 and 71 bases, a list of 256 primers with winners in every
    lane round and a copy that loses to the lower index, a list of one, the
    two lists in one file (tests/primer_cases.py: directed_fastq)."""
    lists = primer_cases.directed_primers()
    want, stats, n, total = primer_cases.directed_expected()
    got, result, summary, _ = _trim_bytes(primer_cases.directed_fastq(), lists)
    assert got == want
    assert primer_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_one_primer_wins_5000_records():
    """Every block adds to the same two statistics slots."""
    one = primer_oracle.trim_bytes(primer_cases.record(0, 2, P + 'GATTACA').encode(), [], [P], E)
    assert one[1] == {(2, 0): [1, 22]}
    data = ''.join(primer_cases.record(i, 2, P + 'GATTACA') for i in range(5000)).encode()
    got, result, _, _ = _trim_bytes(data, ([], [P]))
    assert got == ''.join(primer_cases.record(i, 2, 'GATTACA', qual=primer_cases.record(i, 2, P + 'GATTACA')
                                              .split('\n')[3][22:]) for i in range(5000)).encode()
    assert primer_cases.stats_of(result) == {(2, 0): [5000, 5000 * 22]}


@pytest.mark.parametrize('path', ['streamed', 'bytes'])
@pytest.mark.parametrize('use_gzip', [True, False])
def test_fuzz_file(tmp_path, use_gzip, path):
    """About 4000 records, 96 primers a direction, through the file-to-file
    streamed path and through bytes, gzip and plain: byte-equal to the oracle
    after decompression, equal statistics (the file's make-up is checked in
    tests/test_primer_oracle.py)."""
    data = primer_cases.fuzz_fastq()
    lists = primer_cases.fuzz_primers()
    want, stats, n, total, _ = primer_cases.fuzz_expected()
    if path == 'bytes':
        got, result, summary, _ = _trim_bytes(data, lists, use_gzip=use_gzip)
    else:
        src_path, dst_path = tmp_path / 'in.fastq', tmp_path / 'out.fastq'
        src_path.write_bytes(gzip.compress(data, 1) if use_gzip else data)
        summary = io.StringIO()
        with open(src_path, 'rb') as src, open(dst_path, 'wb') as dst:
            result = trim_fastqs.trim(src, dst, (), use_gzip=use_gzip, summary_file=summary,
                                      primers1=lists[0], primers2=lists[1])
        got, summary = dst_path.read_bytes(), summary.getvalue()
        if use_gzip:
            got = gzip.decompress(got)
    assert got == want
    assert primer_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_fuzz_file_censor_then_primers():
    """Bad cycles first: a bad cycle inside the primer is an 'N' and counts
    as an error, and base_count and score_sum are the censor-only values."""
    want, stats, n, total, _ = primer_cases.fuzz_expected(True)
    assert (n, total) == primer_cases.fuzz_expected()[2:4]
    assert want != primer_cases.fuzz_expected()[0]
    got, result, summary, _ = _trim_bytes(primer_cases.fuzz_fastq(), primer_cases.fuzz_primers(),
                                          bad_cycles_reader=trim_cases.fuzz_bad_rows())
    assert got == want
    assert primer_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_adapters_and_primers_in_one_call():
    """The primers are looked for in what the adapters left: a cut below the
    primer's reach, a read trimmed at both ends, the two trims meeting in an
    empty record."""
    want, adapter_stats, primer_stats = primer_cases.both_ends_expected()
    got, result, _, _ = _trim_bytes(primer_cases.both_ends_fastq(), ([P], None),
                                    adapters=(primer_cases.ADAPTER, None), min_overlap=trim_cases.MIN_OVERLAP)
    assert got == want
    lines = got.split(b'\n')
    assert lines[1].decode() == P[:10] and lines[5].decode() == primer_cases.INSERT[:40]
    assert lines[9] == lines[11] == b''
    assert trim_cases.stats_of(result) == adapter_stats
    assert primer_cases.stats_of(result) == primer_stats


def test_read_past_the_adapter_cap_passes_with_primers_only():
    long_read = P + 'ACGT' * 17500
    data = '@M1:2:F:1:1101:7:70000 1:N:0:1\n{}\n+\n{}\n'.format(long_read, 'F' * len(long_read)).encode()
    got, result, _, _ = _trim_bytes(data, ([P], None))
    assert got == '@M1:2:F:1:1101:7:70000 1:N:0:1\n{}\n+\n{}\n'.format('ACGT' * 17500, 'F' * 70000).encode()
    assert result['primer_reads'] == 1 and result['primer_bases'] == 22
    with pytest.raises(_native.NativeError, match=r'record 1 \(@M1:2:F:1:1101:7:70000\)'):
        _trim_bytes(data, ([P], None), adapters=('nextera', None))


def test_primers_are_cleared_after_the_call():
    G = json.load(open(os.path.join(HERE, 'golden', 'censor', 'censor_golden.json')))
    data = primer_cases.record(0, 1, P + 'GATTACA').encode()
    got, result, _, _ = _trim_bytes(data, ([P], None))
    assert result['primer_reads'] == 1 and got.split(b'\n')[1] == b'GATTACA'
    dest = io.BytesIO()
    censor_fastq.censor(io.BytesIO(data), [], dest, use_gzip=False)
    assert dest.getvalue() == data
    for case in G['cases']:
        dest, summary = io.BytesIO(), io.StringIO()
        censor_fastq.censor(io.BytesIO(case['fastq'].encode()),
                            [dict(tile=t, cycle=c) for t, c in case['bad_cycles']], dest,
                            use_gzip=False, summary_file=summary)
        assert dest.getvalue().decode() == case['censored']
        assert summary.getvalue() == case['summary']
    assert session.context().censor_primer_stats() == ([[0] * 256] * 2, [[0] * 256] * 2)


def test_library_refuses_bad_primers():
    ctx = session.context()
    for args in ((['ACGTACG'], [], E), ([P[:10] + 'R' + P[11:]], [], E), ([], ['A' * 65], E),
                 (['ACGTACGT'] * 257, [], E), ([P.lower()], [], E), ([P], [], list(range(65))),
                 ([P], [], [0] * 64 + [64]), ([P], [], [-1] + [0] * 64)):
        with pytest.raises(_native.NativeError, match=r'\(-3\)'):
            ctx.censor_set_primers(*args)
    with pytest.raises(_native.NativeError, match='primer 1 of read direction 2'):
        ctx.censor_set_primers([P], [P, P[:10] + 'R' + P[11:]], E)
    ctx.censor_set_primers([P] * 256, [], primer_oracle.error_table(0.98))
    ctx.censor_clear_primers()


def test_command_line(tmp_path, capsys):
    data = primer_cases.directed_fastq()
    lists = primer_cases.directed_primers()
    src, dst, fasta = tmp_path / 'in.fastq.gz', tmp_path / 'out.fastq.gz', tmp_path / 'scheme.fasta'
    src.write_bytes(gzip.compress(data, 1))
    fasta.write_text(''.join('>amplicon_{}_LEFT\n{}\n'.format(k, p) for k, p in enumerate(lists[0])))
    trim_fastqs.main([str(src), str(dst), '--primers', str(fasta), '--primers2', lists[1][0],
                      '--summary', str(tmp_path / 'summary.csv'), '--primer-summary', str(tmp_path / 'primers.csv')])
    want, stats, n, total = primer_cases.directed_expected()
    assert gzip.decompress(dst.read_bytes()) == want
    assert capsys.readouterr().out == 'direction,adapter,reads,bases\n'
    rows = list(csv.DictReader(io.StringIO((tmp_path / 'primers.csv').read_text())))
    names = ['amplicon_{}_LEFT'.format(k) for k in range(256)] + ['primer1']
    assert [(int(r['direction']), r['name'], r['primer'], [int(r['reads']), int(r['bases'])]) for r in rows] == \
        [(d, names[256 * (d - 1) + k], p, stats.get((d, k), [0, 0]))
         for d in (1, 2) for k, p in enumerate(lists[d - 1])]
    assert (tmp_path / 'summary.csv').read_text() == _summary(n, total)


def test_adapters_only_is_unchanged():
    """Without primers no lead is set: the writer's output and the returned
    statistics are those of the 3' trimming alone."""
    want, stats, n, total, _ = trim_cases.fuzz_expected()
    dest, summary = io.BytesIO(), io.StringIO()
    result = trim_fastqs.trim(io.BytesIO(trim_cases.fuzz_fastq()), dest, *trim_cases.FUZZ_ADAPTERS,
                              use_gzip=False, summary_file=summary, min_overlap=trim_cases.MIN_OVERLAP)
    assert dest.getvalue() == want
    assert trim_cases.stats_of(result) == stats
    assert summary.getvalue() == _summary(n, total)
    assert (result['primer_reads'], result['primer_bases'], result['primers']) == (0, 0, [])

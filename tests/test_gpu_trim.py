"""3' adapter trimming on the device (micall_amd.trim_fastqs, k_trim in
csrc/mh_censor.hip) against tests/trim_oracle.py applied to what
oracle/og_censor.py makes of the same file: directed records, one fuzz file
through every path of the drop-in, bad cycles first, the read-length cap,
and the adapters cleared after the call."""
import csv
import gzip
import io
import json
import os

import pytest

import trim_cases
import trim_oracle
from micall_amd import _native, censor_fastq, session, trim_fastqs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _trim_bytes(data, lists, use_gzip=False, **kwargs):
    dest, summary, trim_summary = io.BytesIO(), io.StringIO(), io.StringIO()
    result = trim_fastqs.trim(io.BytesIO(gzip.compress(data, 1) if use_gzip else data), dest, lists[0], lists[1],
                              use_gzip=use_gzip, summary_file=summary, trim_summary_file=trim_summary,
                              min_overlap=trim_cases.MIN_OVERLAP, **kwargs)
    out = dest.getvalue()
    return (gzip.decompress(out) if use_gzip else out), result, summary.getvalue(), trim_summary.getvalue()


def _summary(n, total):
    return 'avg_quality,base_count\n{},{}\n'.format(repr(total / n), n)


@pytest.mark.parametrize('count', [1, 8])
def test_directed_records(count):
    """Read lengths 0 .. 700 across the 64-column blocks of the kernel,
    adapters of 3, 19, 33 and 64 bases, 1 and 8 per list, different lists for
    the two directions in one file (tests/trim_cases.py: directed_fastq)."""
    lists = trim_cases.directed_adapters(count)
    want, stats, n, total = trim_cases.directed_expected(count)
    got, result, summary, _ = _trim_bytes(trim_cases.directed_fastq(count), lists)
    assert got == want
    assert trim_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_directed_literals():
    """The values the rules were checked on, on the device: a 19-base
    adapter at rate 0.1 after a 100-base insert."""
    a = trim_cases.NEXTERA
    insert = 'GATTACA' * 14 + 'GG'
    reads = [insert + a + 'GATTACAG', insert + a[:9] + 'G' + a[10:] + 'GATTACAG',
             insert + a[:9] + a[10:] + 'GATTACAG', insert + a[:9] + 'G' + a[9:] + 'GATTACAG',
             insert + a[:10], insert + a[:3], insert + a[:2], insert, a + insert, a, '']
    kept = [100, 100, 100, 100, 100, 100, 102, 100, 0, 0, 0]
    data = ''.join(trim_cases.record(i, 1 + i % 2, r) for i, r in enumerate(reads)).encode()
    got, result, _, trim_summary = _trim_bytes(data, ('nextera', None))
    lines = got.split(b'\n')
    assert [len(lines[4 * i + 1]) for i in range(len(reads))] == kept
    assert [len(lines[4 * i + 3]) for i in range(len(reads))] == kept
    assert got == trim_oracle.trim_bytes(data, [a], [a], 3, trim_cases.E)[0]
    assert result['reads'] == 8 and result['bases'] == 27 + 27 + 26 + 28 + 10 + 3 + 119 + 19
    rows = list(csv.DictReader(io.StringIO(trim_summary)))
    assert rows == [dict(direction=str(d), adapter=a, reads='4', bases=str(b))
                    for d, b in ((1, 27 + 26 + 10 + 119), (2, 27 + 28 + 3 + 19))]


@pytest.mark.parametrize('path', ['streamed', 'bytes'])
@pytest.mark.parametrize('use_gzip', [True, False])
def test_fuzz_file(tmp_path, use_gzip, path):
    """About 4000 records through the file-to-file streamed path and through
    bytes, gzip and plain: byte-equal to the oracle after decompression, equal
    statistics; by the oracle each of the classes full, partial and
    untrimmed holds at least a fifth of the records."""
    data = trim_cases.fuzz_fastq()
    want, stats, n, total, classes = trim_cases.fuzz_expected()
    records = sum(classes.values())
    assert 3900 <= records <= 4100 and set(classes) == {'full', 'partial', 'untrimmed'}
    assert all(5 * v >= records for v in classes.values()), classes
    if path == 'bytes':
        got, result, summary, _ = _trim_bytes(data, trim_cases.FUZZ_ADAPTERS, use_gzip=use_gzip)
    else:
        src_path, dst_path = tmp_path / 'in.fastq', tmp_path / 'out.fastq'
        src_path.write_bytes(gzip.compress(data, 1) if use_gzip else data)
        summary = io.StringIO()
        with open(src_path, 'rb') as src, open(dst_path, 'wb') as dst:
            result = trim_fastqs.trim(src, dst, *trim_cases.FUZZ_ADAPTERS, use_gzip=use_gzip,
                                      summary_file=summary, min_overlap=trim_cases.MIN_OVERLAP)
        got, summary = dst_path.read_bytes(), summary.getvalue()
        if use_gzip:
            got = gzip.decompress(got)
    assert got == want
    assert trim_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_fuzz_file_censor_then_trim():
    """Bad cycles first: the adapters are looked for in the censored line
    (bad cycles 'N', the trailing bad run gone), and base_count and
    score_sum are the censor-only values."""
    want, stats, n, total, _ = trim_cases.fuzz_expected(True)
    assert (n, total) == trim_cases.fuzz_expected()[2:4]
    assert want != trim_cases.fuzz_expected()[0]
    got, result, summary, _ = _trim_bytes(trim_cases.fuzz_fastq(), trim_cases.FUZZ_ADAPTERS,
                                          bad_cycles_reader=trim_cases.fuzz_bad_rows())
    assert got == want
    assert trim_cases.stats_of(result) == stats
    censor_summary = io.StringIO()
    censor_fastq.censor(io.BytesIO(trim_cases.fuzz_fastq()), trim_cases.fuzz_bad_rows(), io.BytesIO(),
                        use_gzip=False, summary_file=censor_summary)
    assert summary == censor_summary.getvalue() == _summary(n, total)


def test_read_past_the_cap_is_named():
    long_read = 'ACGT' * 17500
    data = (trim_cases.record(0, 1, 'ACGTACGT') +
            '@M1:2:F:1:1101:7:70000 1:N:0:1\n{}\n+\n{}\n'.format(long_read, 'F' * len(long_read))).encode()
    with pytest.raises(_native.NativeError, match=r'record 2 \(@M1:2:F:1:1101:7:70000\)'):
        trim_fastqs.trim(io.BytesIO(data), io.BytesIO(), 'nextera', use_gzip=False)
    # only with adapters set: the censor alone takes it
    dest = io.BytesIO()
    censor_fastq.censor(io.BytesIO(data), [], dest, use_gzip=False)
    assert dest.getvalue() == data
    # and a long read that the censor cuts below the cap is taken
    bad = [dict(tile='1101', cycle=str(c)) for c in range(60001, 70001)]
    dest = io.BytesIO()
    result = trim_fastqs.trim(io.BytesIO(data), dest, 'ACGTACGTACGTACGTACGT', bad_cycles_reader=bad,
                              use_gzip=False)
    assert dest.getvalue().split(b'\n')[5] == b'' and result['bases'] == 8 + 60000


def test_adapters_are_cleared_after_the_call():
    G = json.load(open(os.path.join(HERE, 'golden', 'censor', 'censor_golden.json')))
    case = G['cases'][0]
    trimmed = io.BytesIO()
    result = trim_fastqs.trim(io.BytesIO(case['fastq'].encode()), trimmed, 'CGTA', use_gzip=False)
    assert result['reads'] >= 1 and trimmed.getvalue().decode() != case['censored']
    for case in G['cases']:
        dest, summary = io.BytesIO(), io.StringIO()
        censor_fastq.censor(io.BytesIO(case['fastq'].encode()),
                            [dict(tile=t, cycle=c) for t, c in case['bad_cycles']], dest,
                            use_gzip=False, summary_file=summary)
        assert dest.getvalue().decode() == case['censored']
        assert summary.getvalue() == case['summary']
    assert session.context().censor_trim_stats() == ([[0] * 8] * 2, [[0] * 8] * 2)


def test_library_refuses_bad_adapters():
    ctx = session.context()
    E = trim_cases.E
    for args in ((['AC'], [], 3, E), (['ACGN'], [], 3, E), ([], ['A' * 65], 3, E), (['ACG'] * 9, [], 3, E),
                 (['ACGT'], [], 0, E), (['ACGT'], [], 3, list(range(65)))):
        with pytest.raises(_native.NativeError, match=r'\(-3\)'):
            ctx.censor_set_adapters(*args)
    ctx.censor_clear_adapters()


def test_command_line(tmp_path, capsys):
    data = trim_cases.directed_fastq(1)
    lists = trim_cases.directed_adapters(1)
    src, dst = tmp_path / 'in.fastq.gz', tmp_path / 'out.fastq.gz'
    src.write_bytes(gzip.compress(data, 1))
    trim_fastqs.main([str(src), str(dst), '--adapters', lists[0][0], '--adapters2', lists[1][0],
                      '--summary', str(tmp_path / 'summary.csv')])
    want, stats, n, total = trim_cases.directed_expected(1)
    assert gzip.decompress(dst.read_bytes()) == want
    rows = list(csv.DictReader(io.StringIO(capsys.readouterr().out)))
    assert [(int(r['direction']), r['adapter'], [int(r['reads']), int(r['bases'])]) for r in rows] == \
        [(1, lists[0][0], stats[(1, 0)]), (2, lists[1][0], stats[(2, 0)])]
    assert (tmp_path / 'summary.csv').read_text() == _summary(n, total)

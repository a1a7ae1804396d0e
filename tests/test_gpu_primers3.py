"""3' primer trimming on the device (micall_amd.trim_fastqs, k_primer3 in
csrc/mh_censor.hip) against tests/primer3_oracle.py applied to what
oracle/og_censor.py (and tests/trim_oracle.py and tests/primer_oracle.py, with
adapters and 5' primers) make of the same file: the literal cases, directed
records, matches at the 5' primer's lead, one fuzz file through every path of
the drop-in, bad cycles, adapters, 5' and 3' primers in one call, a read past
the cap, the lists cleared after the call, the library's refusals, the
command line, and nothing changed or launched without a 3' list."""
import csv
import gzip
import io
import json
import os

import pytest

import primer3_cases
import primer3_oracle
import primer_cases
import trim_cases
from micall_amd import _native, censor_fastq, session, trim_fastqs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
P, E, MIN_OVERLAP = primer3_cases.P, primer3_cases.E, primer3_cases.MIN_OVERLAP


def _trim_bytes(data, primers3, primers=(None, None), adapters=((), None), use_gzip=False, **kwargs):
    dest, summary, primer3_summary = io.BytesIO(), io.StringIO(), io.StringIO()
    result = trim_fastqs.trim(io.BytesIO(gzip.compress(data, 1) if use_gzip else data), dest, adapters[0],
                              adapters[1], use_gzip=use_gzip, summary_file=summary, primers1=primers[0],
                              primers2=primers[1], primers3_1=primers3[0], primers3_2=primers3[1],
                              primer3_summary_file=primer3_summary, **kwargs)
    out = dest.getvalue()
    return (gzip.decompress(out) if use_gzip else out), result, summary.getvalue(), primer3_summary.getvalue()


def _summary(n, total):
    return 'avg_quality,base_count\n{},{}\n'.format(repr(total / n), n)


def test_literals():
    """The values the rules were checked on, on the device: a 22-base primer
    at rate 0.1 and min_overlap 12 behind a 70-base insert."""
    data = primer3_cases.literals_fastq()
    got, result, _, primer3_summary = _trim_bytes(data, ([P], [P]))
    lines, src = got.split(b'\n'), data.split(b'\n')
    for i, (name, read, cut, _, _) in enumerate(primer3_cases.LITERALS):
        assert lines[4 * i + 1].decode() == read[:len(read) - (cut or 0)], name
        assert lines[4 * i + 3] == src[4 * i + 3][:len(read) - (cut or 0)], name
        assert lines[4 * i] == src[4 * i] and lines[4 * i + 2] == b'+'
    want, stats = primer3_oracle.trim_bytes(data, None, [P], [P], E, MIN_OVERLAP)
    assert got == want and primer3_cases.stats_of(result) == stats
    cuts = [cut for _, _, cut, _, _ in primer3_cases.LITERALS]
    assert result['primer3_reads'] == sum(x is not None for x in cuts)
    assert result['primer3_bases'] == sum(x or 0 for x in cuts)
    assert result['reads'] == result['bases'] == 0 and result['adapters'] == []
    assert result['primer_reads'] == result['primer_bases'] == 0 and result['primers'] == []
    rows = list(csv.DictReader(io.StringIO(primer3_summary)))
    assert rows == [dict(direction=str(d), name='primer1', primer=P, reads=str(stats[(d, 0)][0]),
                         bases=str(stats[(d, 0)][1])) for d in (1, 2)]
    # the longer of two matching primers wins, of two equal ones the first
    one = primer3_cases.record(0, 1, primer3_cases.INSERT + P).encode()
    assert primer3_cases.stats_of(_trim_bytes(one, ([P[8:], P], None))[1]) == {(1, 1): [1, 22]}
    assert primer3_cases.stats_of(_trim_bytes(one, ({'a': P, 'b': P}, None))[1]) == {(1, 0): [1, 22]}
    # min_overlap is the call's: at 14 the 12 bases at the end stay (at 13 they go with one more, cost 1)
    short = primer3_cases.record(0, 1, primer3_cases.INSERT + P[:12]).encode()
    assert _trim_bytes(short, ([P], None), primer3_min_overlap=14)[0] == short
    assert _trim_bytes(short, ([P], None))[1]['primer3_bases'] == 12


def test_directed_records():
    """Primers of 8 and 64 bases, texts of 0, 1, 11, 12, 63, 64, 65, 127,
    128, 129 and 300 bases, a partial match of 63 bases, matches on the
    block boundaries of the backward scan, an N and a lower-case base, a full
    and a partial candidate with equal L - D, a list of 256 primers with
    winners in every lane round and a copy that loses to the lower index,
    another list for the other direction (tests/primer3_cases.py:
    directed_fastq)."""
    lists = primer3_cases.directed_primers()
    want, stats, n, total, _ = primer3_cases.directed_expected()
    got, result, summary, _ = _trim_bytes(primer3_cases.directed_fastq(), lists)
    assert got == want
    assert primer3_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_matches_at_the_lead():
    """Behind a 5' primer: a 3' match that starts exactly at the lead is
    found, one that starts a base before it is found only without that
    base, and a cut never falls before the lead."""
    want, stats5, stats3, _, _ = primer3_cases.lead_expected()
    lists3 = primer3_cases.LEAD_PRIMERS3
    got, result, _, _ = _trim_bytes(primer3_cases.lead_fastq(), (lists3, lists3), primers=([primer3_cases.P5], None))
    assert got == want
    assert primer_cases.stats_of(result) == stats5
    assert primer3_cases.stats_of(result) == stats3


def test_mates():
    """'mates': read 1 is searched for the reverse complements of the
    primers read 2 begins with, and read 2 for those of read 1."""
    five = primer3_cases.CHAIN_PRIMERS
    rc = primer3_cases.reverse_complement
    reads = [(1, five[0][0] + primer3_cases.INSERT + rc(five[1][1]) + 'GATTACA'),
             (2, five[1][1] + rc(primer3_cases.INSERT) + rc(five[0][0])),
             (1, five[0][1] + primer3_cases.INSERT + five[1][0]),          # not reverse-complemented: stays
             (2, five[1][0] + primer3_cases.INSERT + rc(five[1][0]))]      # its own primer's: stays
    data = ''.join(primer3_cases.record(i, d, r) for i, (d, r) in enumerate(reads)).encode()
    got, result, _, _ = _trim_bytes(data, ('mates', 'mates'), primers=five)
    assert [ln.decode() for ln in got.split(b'\n')[1::4]] == \
        [primer3_cases.INSERT, rc(primer3_cases.INSERT), primer3_cases.INSERT + five[1][0],
         primer3_cases.INSERT + rc(five[1][0])]
    assert result['primers3'] == [
        dict(direction=1, name='primer1', primer=rc(five[1][0]), reads=0, bases=0),
        dict(direction=1, name='primer2', primer=rc(five[1][1]), reads=1, bases=len(five[1][1]) + 7),
        dict(direction=2, name='primer1', primer=rc(five[0][0]), reads=1, bases=len(five[0][0])),
        dict(direction=2, name='primer2', primer=rc(five[0][1]), reads=0, bases=0)]
    # one side only
    got, result, _, _ = _trim_bytes(data, (None, 'mates'), primers=five)
    assert got.split(b'\n')[1].decode() == primer3_cases.INSERT + rc(five[1][1]) + 'GATTACA'
    assert [r['direction'] for r in result['primers3']] == [2, 2] and result['primer3_reads'] == 1


def test_one_primer_wins_5000_records():
    """Every block adds to the same two statistics slots."""
    data = ''.join(primer3_cases.record(i, 2, 'GATTACA' + P + 'TG') for i in range(5000)).encode()
    got, result, _, _ = _trim_bytes(data, (None, [P]))
    assert got == ''.join(primer3_cases.record(i, 2, 'GATTACA', qual=primer3_cases.record(i, 2, 'GATTACA' + P + 'TG')
                                               .split('\n')[3][:7]) for i in range(5000)).encode()
    assert primer3_cases.stats_of(result) == {(2, 0): [5000, 5000 * 24]}


@pytest.mark.parametrize('path', ['streamed', 'bytes'])
@pytest.mark.parametrize('use_gzip', [True, False])
def test_fuzz_file(tmp_path, use_gzip, path):
    """About 4000 records of 60 to 160 bases, 96 primers a direction, through
    the file-to-file streamed path and through bytes, gzip and plain:
    byte-equal to the oracle after decompression, equal statistics, and a
    tenth of the file at least in each of the oracle's classes."""
    data = primer3_cases.fuzz_fastq()
    lists = primer3_cases.fuzz_primers()
    want, stats, n, total, classes = primer3_cases.fuzz_expected()
    assert set(classes) == {'full exact', 'full errors', 'partial', 'untrimmed'}
    assert all(10 * v >= sum(classes.values()) for v in classes.values()), classes
    if path == 'bytes':
        got, result, summary, _ = _trim_bytes(data, lists, use_gzip=use_gzip)
    else:
        src_path, dst_path = tmp_path / 'in.fastq', tmp_path / 'out.fastq'
        src_path.write_bytes(gzip.compress(data, 1) if use_gzip else data)
        summary = io.StringIO()
        with open(src_path, 'rb') as src, open(dst_path, 'wb') as dst:
            result = trim_fastqs.trim(src, dst, (), use_gzip=use_gzip, summary_file=summary,
                                      primers3_1=lists[0], primers3_2=lists[1])
        got, summary = dst_path.read_bytes(), summary.getvalue()
        if use_gzip:
            got = gzip.decompress(got)
    assert got == want
    assert primer3_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_fuzz_file_censor_then_primers3():
    """Bad cycles first: a bad cycle inside the primer is an 'N' and counts
    as an error, a dropped trailing run moves the read's end, and base_count
    and score_sum are the censor-only values."""
    want, stats, n, total, _ = primer3_cases.fuzz_expected(True)
    assert (n, total) == primer3_cases.fuzz_expected()[2:4]
    assert want != primer3_cases.fuzz_expected()[0]
    got, result, summary, _ = _trim_bytes(primer3_cases.fuzz_fastq(), primer3_cases.fuzz_primers(),
                                          bad_cycles_reader=trim_cases.fuzz_bad_rows())
    assert got == want
    assert primer3_cases.stats_of(result) == stats
    assert summary == _summary(n, total)


def test_bad_cycles_adapters_and_both_primers_in_one_call():
    """The 3' search sees what the three passes before left: the bad cycles
    as 'N', the read cut at the adapter, the text from the 5' primer's lead."""
    want, adapter_stats, stats5, stats3, n, total = primer3_cases.chain_expected()
    got, result, summary, _ = _trim_bytes(primer3_cases.chain_fastq(), ('mates', 'mates'),
                                          primers=primer3_cases.CHAIN_PRIMERS,
                                          adapters=(primer3_cases.ADAPTER, None),
                                          min_overlap=trim_cases.MIN_OVERLAP,
                                          bad_cycles_reader=trim_cases.fuzz_bad_rows())
    assert got == want
    assert trim_cases.stats_of(result) == adapter_stats
    assert primer_cases.stats_of(result) == stats5
    assert primer3_cases.stats_of(result) == stats3
    assert summary == _summary(n, total)


def test_read_past_the_cap_fails_by_name():
    long_read = 'ACGT' * 17500 + P
    data = '@M1:2:F:1:1101:7:70000 1:N:0:1\n{}\n+\n{}\n'.format(long_read, 'F' * len(long_read)).encode()
    with pytest.raises(_native.NativeError, match=r'record 1 \(@M1:2:F:1:1101:7:70000\)'):
        _trim_bytes(data, ([P], None))
    # the longest read there is room for
    fits = 'ACGT' * 16378 + P + 'G'
    assert len(fits) == 65535
    data = '@M1:2:F:1:1101:7:65535 1:N:0:1\n{}\n+\n{}\n'.format(fits, 'F' * len(fits)).encode()
    got, result, _, _ = _trim_bytes(data, ([P], None))
    assert got == '@M1:2:F:1:1101:7:65535 1:N:0:1\n{}\n+\n{}\n'.format('ACGT' * 16378, 'F' * 65512).encode()
    assert (result['primer3_reads'], result['primer3_bases']) == (1, 23)


def test_primers3_are_cleared_after_the_call():
    G = json.load(open(os.path.join(HERE, 'golden', 'censor', 'censor_golden.json')))
    data = primer3_cases.record(0, 1, 'GATTACA' + P).encode()
    got, result, _, _ = _trim_bytes(data, ([P], None))
    assert result['primer3_reads'] == 1 and got.split(b'\n')[1] == b'GATTACA'
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
    assert session.context().censor_primer3_stats() == ([[0] * 256] * 2, [[0] * 256] * 2)
    # a call that fails clears them too
    with pytest.raises(_native.NativeError):
        _trim_bytes(b'@no header\nACGT\n+\n', ([P], None))
    dest = io.BytesIO()
    censor_fastq.censor(io.BytesIO(data), [], dest, use_gzip=False)
    assert dest.getvalue() == data


def test_library_refuses_bad_primers3():
    ctx = session.context()
    for args in ((['ACGTACG'], [], 12, E), ([P[:10] + 'R' + P[11:]], [], 12, E), ([], ['A' * 65], 12, E),
                 (['ACGTACGT'] * 257, [], 12, E), ([P.lower()], [], 12, E), ([P], [], 12, list(range(65))),
                 ([P], [], 12, [0] * 64 + [64]), ([P], [], 12, [-1] + [0] * 64), ([P], [], 0, E),
                 ([P], [], 65, E), ([P], [], -3, E)):
        with pytest.raises(_native.NativeError, match=r'\(-3\)'):
            ctx.censor_set_primers3(*args)
    with pytest.raises(_native.NativeError, match="3' primer 1 of read direction 2"):
        ctx.censor_set_primers3([P], [P, P[:10] + 'R' + P[11:]], 12, E)
    with pytest.raises(_native.NativeError, match='min_overlap 65'):
        ctx.censor_set_primers3([P], [], 65, E)
    ctx.censor_set_primers3([P] * 256, [], 64, primer3_oracle.error_table(0.98))
    ctx.censor_set_primers3([P], [], 1, E)
    ctx.censor_clear_primers3()


def test_command_line(tmp_path, capsys):
    data = primer3_cases.directed_fastq()
    lists = primer3_cases.directed_primers()
    src, dst, fasta = tmp_path / 'in.fastq.gz', tmp_path / 'out.fastq.gz', tmp_path / 'scheme.fasta'
    src.write_bytes(gzip.compress(data, 1))
    fasta.write_text(''.join('>amplicon_{}_RIGHT\n{}\n'.format(k, p) for k, p in enumerate(lists[0])))
    # --primers3 alone, without --adapters or --primers
    trim_fastqs.main([str(src), str(dst), '--primers3', str(fasta), '--primers3-2', ','.join(lists[1]),
                      '--summary', str(tmp_path / 'summary.csv'), '--primer3-summary', str(tmp_path / 'primers3.csv')])
    want, stats, n, total, _ = primer3_cases.directed_expected()
    assert gzip.decompress(dst.read_bytes()) == want
    assert capsys.readouterr().out == 'direction,adapter,reads,bases\n'
    rows = list(csv.DictReader(io.StringIO((tmp_path / 'primers3.csv').read_text())))
    names = ['amplicon_{}_RIGHT'.format(k) for k in range(256)] + ['primer{}'.format(k + 1) for k in range(5)]
    assert [(int(r['direction']), r['name'], r['primer'], [int(r['reads']), int(r['bases'])]) for r in rows] == \
        [(d, names[256 * (d - 1) + k], p, stats.get((d, k), [0, 0]))
         for d in (1, 2) for k, p in enumerate(lists[d - 1])]
    assert (tmp_path / 'summary.csv').read_text() == _summary(n, total)
    # 'mates' and --primer3-min-overlap
    five = primer3_cases.CHAIN_PRIMERS
    read = five[0][0] + primer3_cases.INSERT + primer3_cases.reverse_complement(five[1][0])[:13]
    plain, out = tmp_path / 'one.fastq', tmp_path / 'one.out.fastq'
    plain.write_text(primer3_cases.record(0, 1, read))
    base = [str(plain), str(out), '--unzipped', '--primers', ','.join(five[0]), '--primers2', ','.join(five[1]),
            '--primers3', 'mates']
    trim_fastqs.main(base)
    assert out.read_text().split('\n')[1] == primer3_cases.INSERT
    trim_fastqs.main(base + ['--primer3-min-overlap', '20'])
    assert out.read_text().split('\n')[1] == read[len(five[0][0]):]
    with pytest.raises(SystemExit):
        trim_fastqs.main([str(plain), str(out)])


def test_without_a_3_prime_list_nothing_changes_and_nothing_is_launched():
    """The output of trim() without a 3' list is byte-equal to that of a call
    that never heard of the feature (the oracles of the earlier passes), and
    the context's profile holds no k_primer3 entry; with a list it does."""
    ctx = session.context()
    want, stats, n, total, _ = trim_cases.fuzz_expected()
    pwant, pstats = primer_cases.fuzz_expected()[:2]
    ctx.profile(True)
    try:
        dest, summary = io.BytesIO(), io.StringIO()
        result = trim_fastqs.trim(io.BytesIO(trim_cases.fuzz_fastq()), dest, *trim_cases.FUZZ_ADAPTERS,
                                  use_gzip=False, summary_file=summary, min_overlap=trim_cases.MIN_OVERLAP)
        assert dest.getvalue() == want
        assert trim_cases.stats_of(result) == stats
        assert summary.getvalue() == _summary(n, total)
        assert (result['primer3_reads'], result['primer3_bases'], result['primers3']) == (0, 0, [])
        lists = primer_cases.fuzz_primers()
        dest = io.BytesIO()
        result = trim_fastqs.trim(io.BytesIO(primer_cases.fuzz_fastq()), dest, (), use_gzip=False,
                                  primers1=lists[0], primers2=lists[1], primers3_1=None, primers3_2=None)
        assert dest.getvalue() == pwant and primer_cases.stats_of(result) == pstats
        assert result['primers3'] == []
        dest = io.BytesIO()
        censor_fastq.censor(io.BytesIO(primer3_cases.literals_fastq()), [], dest, use_gzip=False)
        assert dest.getvalue() == primer3_cases.literals_fastq()
        assert ctx.profile_get('k_censor')[1] == 3 and ctx.profile_get('k_trim')[1] == 1
        assert ctx.profile_get('k_primer')[1] == 1
        assert ctx.profile_get('k_primer3')[1] == 0
        _trim_bytes(primer3_cases.literals_fastq(), ([P], [P]))
        assert ctx.profile_get('k_primer3')[1] == 1 and ctx.profile_get('k_censor')[1] == 4
        assert ctx.profile_get('k_trim')[1] == 1 and ctx.profile_get('k_primer')[1] == 1
    finally:
        ctx.profile(False)

"""Every row-output route of the context gives the same bytes: format_rows,
format_rows_bytes, write_rows (descriptor path and stream path),
write_rows_at and format_segments + write_segments, as SAM (style 0) and CSV
(style 1), for all reads and for an order.

40,000 unpaired reads is the smallest input the chunked formatter cuts in
three at 16 threads ((40000 >> 14) + 1 chunks, bounds at rows 13,333 and
26,666); the streaming writer cuts it in ten.  The expected text is made
without the library's formatter: the device's own records through the
oracle's sam_fields (style 0) and its first eleven fields through csv.writer
(style 1)."""
import csv
import io
import os
import zlib

import numpy as np
import pytest

import oracle
from micall_amd import _native, projects

pytestmark = pytest.mark.gpu

POL = projects.load_default().seed_sequences()['HIV1B-pol-seed']
N = 40000
READ_LEN = 50
REFNAMES = ['POL']
CSV_HEAD = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'


def _inputs():
    rng = np.random.default_rng(41)
    seqs, quals, names = [], [], []
    starts = rng.integers(0, len(POL) - READ_LEN, N)
    random_bases = rng.integers(0, 4, (N, READ_LEN))
    # Phred 1 .. 40: '"' (Phred 1) and ',' (Phred 11) occur, so CSV quotes QUAL
    phred = rng.integers(1, 41, (N, READ_LEN))
    for i in range(N):
        if i % 2:
            seqs.append(''.join('ACGT'[b] for b in random_bases[i]))   # stays unmapped
        else:
            seqs.append(POL[starts[i]:starts[i] + READ_LEN])
        quals.append(''.join(chr(33 + q) for q in phred[i]))
        names.append('read{}'.format(i))
    for i, odd in ((0, 'a,b'), (13333, 'say "hi"'), (13334, '",'), (26666, 'x,"y",z'), (N - 1, 'end,')):
        names[i] = odd
    return names, seqs, quals


@pytest.fixture(scope='module')
def mapped():
    """(context with the reads mapped, expected lines per style)"""
    names, seqs, quals = _inputs()
    ctx = _native.Context(0)
    try:
        ctx.index_build(REFNAMES, [POL], oracle.seed_len(oracle.LOCAL))
        ctx.reads_load(seqs, quals, False, names=names)
        ctx.map(_native.params(oracle.LOCAL))
        alns = ctx.fetch()
        assert 0.3 < (alns['flag'] & 4 == 0).mean() < 0.7   # mapped and unmapped rows
        sam, rows = [], []
        for i in range(N):
            a = oracle.OgAln.from_buffer_copy(alns[i].tobytes())
            f = oracle.sam_fields(a, names[i], seqs[i], quals[i], REFNAMES)
            sam.append(('\t'.join(f) + '\n').encode())
            rows.append(f[:11])
        out = io.StringIO()
        w = csv.writer(out, lineterminator='\n')
        lines_csv = []
        for r in rows:
            w.writerow(r)
            lines_csv.append(out.getvalue().encode())
            out.seek(0)
            out.truncate()
        yield ctx, (sam, lines_csv)
    finally:
        ctx.close()


def _order(which):
    if which == 'all':
        return None
    sub = np.sort(np.random.default_rng(43).choice(N, 30001, replace=False))
    return sub[::-1].copy()


@pytest.fixture(params=[(s, o) for s in (0, 1) for o in ('all', 'order')],
                ids=lambda p: 'style{}-{}'.format(*p))
def case(request, mapped):
    """(context, style, order, expected line list in output order)"""
    ctx, lines = mapped
    style, which = request.param
    order = _order(which)
    picked = lines[style] if order is None else [lines[style][i] for i in order]
    return ctx, style, order, picked


def test_csv_expectation_quotes(mapped):
    """The expected CSV itself: odd names and QUALs are quoted, SAM is not."""
    _, (sam, lines_csv) = mapped
    assert lines_csv[0].startswith(b'"a,b",') and sam[0].startswith(b'a,b\t')
    assert lines_csv[13333].startswith(b'"say ""hi""",')
    assert sum(b'"' in l for l in lines_csv) > N // 2


def test_format_rows(case):
    ctx, style, order, lines = case
    want = b''.join(lines)
    assert ctx.format_rows(style, order=order) == want.decode()
    assert bytes(ctx.format_rows_bytes(style, order=order)) == want


def test_write_rows_text_file(case, tmp_path):
    ctx, style, order, lines = case
    want = b''.join(lines)
    path = tmp_path / 'rows.txt'
    with open(path, 'w', encoding='utf-8') as f:
        assert _native._plain_fd(f) is not None     # the descriptor route
        f.write(CSV_HEAD)
        ctx.write_rows(f, style, order=order)
        assert f.tell() == len(CSV_HEAD) + len(want)
        f.write('tail\n')     # the position is where later writes go
    assert path.read_bytes() == CSV_HEAD.encode() + want + b'tail\n'


def test_write_rows_stream(case):
    ctx, style, order, lines = case
    out = io.StringIO()
    out.write(CSV_HEAD)
    ctx.write_rows(out, style, order=order)
    assert out.getvalue() == CSV_HEAD + b''.join(lines).decode()


def test_write_rows_at(case, tmp_path):
    ctx, style, order, lines = case
    want = b''.join(lines)
    fd = os.open(tmp_path / 'at.bin', os.O_RDWR | os.O_CREAT)
    try:
        written, crc = ctx.write_rows_at(fd, 4097, style, order)
        assert written == len(want)
        assert crc == zlib.crc32(want)
        assert os.fstat(fd).st_size == 4097 + len(want)
        assert os.pread(fd, 4097, 0) == bytes(4097)
        assert os.pread(fd, len(want), 4097) == want
    finally:
        os.close(fd)


def test_write_rows_at_range(case, tmp_path):
    """first / n of write_rows_at select the same rows as format_rows."""
    ctx, style, order, lines = case
    want = b''.join(lines[13000:13000 + 5000])
    fd = os.open(tmp_path / 'range.bin', os.O_RDWR | os.O_CREAT)
    try:
        written, crc = ctx.write_rows_at(fd, 0, style, order, first=13000, n=5000)
        assert (written, crc) == (len(want), zlib.crc32(want))
        assert os.pread(fd, len(want) + 1, 0) == want
    finally:
        os.close(fd)


def test_segments(case, tmp_path):
    ctx, style, order, lines = case
    n = len(lines)
    # empty first and last segments, bounds on and next to both thirds (the
    # chunk bounds of the 40,000-row case)
    bounds = [0, 0, 1, n // 3, n // 3 + 1, 2 * n // 3, n, n]
    if n == N:
        assert bounds == [0, 0, 1, 13333, 13334, 26666, N, N]
    want = [b''.join(lines[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    sizes = ctx.format_segments(style, order, bounds)
    assert [int(x) for x in sizes] == [len(w) for w in want]
    assert int(sizes.sum()) == sum(len(l) for l in lines)
    # the segments in reverse order in the file
    offsets = [int(sizes[k + 1:].sum()) for k in range(len(sizes))]
    fd = os.open(tmp_path / 'seg.bin', os.O_RDWR | os.O_CREAT)
    try:
        crcs = ctx.write_segments(fd, offsets)
        assert os.fstat(fd).st_size == int(sizes.sum())
        for k, w in enumerate(want):
            assert os.pread(fd, len(w), offsets[k]) == w, k
            assert int(crcs[k]) == zlib.crc32(w), k
    finally:
        os.close(fd)

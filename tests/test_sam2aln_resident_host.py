"""session.remap_written / remap_resident: when sam2aln() may take remap.csv's
rows from the device instead of the file (host logic, no GPU: a stub context
and real temporary files)."""
import io
import os

import pytest

from micall_amd import session


class StubContext:
    def __init__(self):
        self.map_serial = 7


ROWS = b'qname,flag\nread1,99\nread1,147\n'


@pytest.fixture
def written(tmp_path, monkeypatch):
    """remap.csv as remap() leaves it: written, recorded with its checksum."""
    import zlib
    monkeypatch.setattr(session, '_key', (('reads.fastq', 1, 2), None))
    monkeypatch.setattr(session, '_remap', None)
    ctx = StubContext()
    path = tmp_path / 'remap.csv'
    with open(path, 'w') as f:
        f.write(ROWS.decode())
        session.remap_written(ctx, f, ['ref-a', 'ref-b'], (zlib.crc32(ROWS), len(ROWS)))
    return ctx, path


def test_unchanged_file_is_resident(written):
    ctx, path = written
    with open(path) as f:
        assert session.remap_resident(ctx, f)
        assert f.tell() == 0
    assert session.remap_refnames() == ['ref-a', 'ref-b']
    with open(path) as f:               # and again, on another handle
        assert session.remap_resident(ctx, f)


def test_touched_file_with_the_same_bytes_is_resident(written):
    ctx, path = written
    path.write_bytes(ROWS)              # same inode, new mtime / ctime
    with open(path) as f:
        assert session.remap_resident(ctx, f)
    session._remap['checksum'] = None   # without a checksum only the identity counts
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_same_size_different_bytes_is_not(written):
    ctx, path = written
    path.write_bytes(ROWS.replace(b'147', b'163'))
    assert os.path.getsize(path) == len(ROWS)
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_other_size_is_not(written):
    ctx, path = written
    path.write_bytes(ROWS.replace(b'\n', b'\r\n'))
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_another_file_with_the_same_bytes_is_not(written, tmp_path):
    ctx, _path = written
    other = tmp_path / 'copy.csv'
    other.write_bytes(ROWS)
    with open(other) as f:
        assert not session.remap_resident(ctx, f)


def test_changed_serial_is_not(written):
    ctx, path = written
    ctx.map_serial += 1                 # another mapping pass or other reads
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_changed_reads_key_is_not(written, monkeypatch):
    ctx, path = written
    monkeypatch.setattr(session, '_key', (('other.fastq', 1, 2), None))
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_invalidate_and_forget_clear_the_record(written):
    ctx, path = written
    session.remap_forget()
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_invalidate_clears_the_record(written, monkeypatch):
    ctx, path = written
    session.invalidate()
    monkeypatch.setattr(session, '_key', (('reads.fastq', 1, 2), None))
    with open(path) as f:
        assert not session.remap_resident(ctx, f)


def test_non_file_handles_are_not(written):
    ctx, path = written
    assert not session.remap_resident(ctx, io.StringIO(ROWS.decode()))
    with open(path, 'rb') as f:         # no text layer: not what readable_fd hands to the parser
        assert not session.remap_resident(ctx, f)


def test_handle_read_from_is_not(written):
    ctx, path = written
    with open(path) as f:
        f.readline()
        assert not session.remap_resident(ctx, f)


def test_record_of_a_non_file_is_never_resident(tmp_path, monkeypatch):
    monkeypatch.setattr(session, '_key', (('reads.fastq', 1, 2), None))
    monkeypatch.setattr(session, '_remap', None)
    ctx = StubContext()
    session.remap_written(ctx, io.StringIO(), ['ref-a'])
    path = tmp_path / 'remap.csv'
    path.write_bytes(ROWS)
    with open(path) as f:
        assert not session.remap_resident(ctx, f)

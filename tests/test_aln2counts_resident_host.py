"""session.aligned_written / aligned_resident: when aln2counts() may count the
rows sam2aln() left on the device instead of parsing aligned.csv (host logic,
no GPU: a stub context and real temporary files)."""
import io
import os
import zlib

import pytest

from micall_amd import session


class StubContext:
    """Only what the record reads: the serial of the sam2aln results.  (No
    map_serial: the record must not depend on the resident reads.)"""

    def __init__(self):
        self.sam2aln_serial = 3


ROWS = b'refname,qcut,rank,count,offset,seq\nHIV1B-pol-seed,15,0,2,0,ACGTAC\n'


@pytest.fixture
def written(tmp_path, monkeypatch):
    """aligned.csv as sam2aln() leaves it: written, recorded with its checksum."""
    monkeypatch.setattr(session, '_key', None)          # no reads resident at all
    monkeypatch.setattr(session, '_aligned', None)
    ctx = StubContext()
    path = tmp_path / 'aligned.csv'
    with open(path, 'w') as f:
        f.write(ROWS.decode())
        session.aligned_written(ctx, f, (zlib.crc32(ROWS), len(ROWS)))
    return ctx, path


def test_unchanged_file_is_resident(written):
    ctx, path = written
    with open(path) as f:
        assert session.aligned_resident(ctx, f)
        assert f.tell() == 0
    with open(path) as f:               # and again, on another handle
        assert session.aligned_resident(ctx, f)


def test_touched_file_with_the_same_bytes_is_resident(written):
    ctx, path = written
    path.write_bytes(ROWS)              # same inode, new mtime / ctime
    with open(path) as f:
        assert session.aligned_resident(ctx, f)
    session._aligned['checksum'] = None   # without a checksum only the identity counts
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_same_size_different_bytes_is_not(written):
    ctx, path = written
    path.write_bytes(ROWS.replace(b'ACGTAC', b'ACGTAA'))
    assert os.path.getsize(path) == len(ROWS)
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_other_size_is_not(written):
    ctx, path = written
    path.write_bytes(ROWS.replace(b'\n', b'\r\n'))
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)
    path.write_bytes(ROWS[:-7] + b'\n')     # truncated inside the last row
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_another_file_with_the_same_bytes_is_not(written, tmp_path):
    ctx, _path = written
    other = tmp_path / 'copy.csv'
    other.write_bytes(ROWS)
    with open(other) as f:
        assert not session.aligned_resident(ctx, f)


def test_changed_serial_is_not(written):
    ctx, path = written
    ctx.sam2aln_serial += 1             # another sam2aln call rebuilt the results
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_the_reads_key_does_not_matter(written, monkeypatch):
    """The sam2aln state owns its data: other reads may be resident by now."""
    ctx, path = written
    monkeypatch.setattr(session, '_key', (('other.fastq', 1, 2), None))
    with open(path) as f:
        assert session.aligned_resident(ctx, f)


def test_forget_clears_the_record(written):
    ctx, path = written
    session.aligned_forget()
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_invalidate_clears_the_record(written):
    ctx, path = written
    session.invalidate()
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_reset_clears_the_record(written, monkeypatch):
    ctx, path = written
    monkeypatch.setattr(session, '_ctx', None)      # nothing to close
    session.reset()
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_non_file_handles_are_not(written):
    ctx, path = written
    assert not session.aligned_resident(ctx, io.StringIO(ROWS.decode()))
    with open(path, 'rb') as f:         # no text layer: not what readable_fd hands to the parser
        assert not session.aligned_resident(ctx, f)


def test_handle_read_from_is_not(written):
    ctx, path = written
    with open(path) as f:
        f.readline()
        assert not session.aligned_resident(ctx, f)


def test_record_of_a_non_file_is_never_resident(tmp_path, monkeypatch):
    monkeypatch.setattr(session, '_aligned', None)
    ctx = StubContext()
    session.aligned_written(ctx, io.StringIO())
    path = tmp_path / 'aligned.csv'
    path.write_bytes(ROWS)
    with open(path) as f:
        assert not session.aligned_resident(ctx, f)


def test_remap_record_still_carries_the_map_serial(tmp_path, monkeypatch):
    """The shared _written helper: remap.csv's record keeps map_serial."""
    class MapStub:
        map_serial = 11

    monkeypatch.setattr(session, '_key', (('reads.fastq', 1, 2), None))
    monkeypatch.setattr(session, '_remap', None)
    with open(tmp_path / 'remap.csv', 'w') as f:
        session.remap_written(MapStub(), f, ['ref-a'])
    assert session._remap['serial'] == 11

"""Host-side rules of the multi-cutoff sam2aln drop-in, no device needed:
the cutoff list's checks come before anything is opened or asked for, a
sharded job with more than one cutoff leaves the split at its first step, and
the cutoff-free (ch, thr) form the merge kernel uses (mh_sam2aln.hip, s2a_pos)
gives merge_pairs' character at every cutoff 0..93."""
import pytest

import og_sam2aln
from micall_amd import sam2aln as s2a
from micall_amd import session


class _Untouchable:
    """Any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError('touched .{}'.format(name))

    def __bool__(self):
        raise AssertionError('tested for truth')


def _no_context(*a, **k):
    raise AssertionError('asked for a context')


def test_sharded_leaves_at_once_with_two_cutoffs(monkeypatch):
    monkeypatch.setattr(session, 'context', _no_context)
    stub = _Untouchable()
    handles = [_Untouchable() for _ in range(4)]
    assert s2a._sam2aln_sharded(stub, *handles, cuts=[15, 10]) is False
    # and with the list taken from the module constant
    monkeypatch.setattr(s2a, 'SAM2ALN_Q_CUTOFFS', [0, 10, 15])
    assert s2a._sam2aln_sharded(stub, *handles) is False


@pytest.mark.parametrize('cuts', [list(range(9)), [15, 10.5], [15, '10'], [], [True]])
def test_bad_cutoff_list_raises_before_any_output(monkeypatch, tmp_path, cuts):
    monkeypatch.setattr(session, 'context', _no_context)
    monkeypatch.setattr(session, 'shard', _no_context)
    with pytest.raises(ValueError):
        s2a.sam2aln(_Untouchable(), _Untouchable(), _Untouchable(), _Untouchable(), q_cutoffs=cuts)
    monkeypatch.setattr(s2a, 'SAM2ALN_Q_CUTOFFS', cuts)
    with pytest.raises(ValueError):
        s2a.sam2aln(_Untouchable(), _Untouchable(), _Untouchable(), _Untouchable())


def test_cutoff_list_drops_repeats_keeping_first(monkeypatch):
    assert s2a._cutoff_list([15, 15]) == [15]
    assert s2a._cutoff_list([15, 10, 15, 0, 10]) == [15, 10, 0]
    assert s2a._cutoff_list(list(range(8)) + [3, 4]) == list(range(8))
    monkeypatch.setattr(s2a, 'SAM2ALN_Q_CUTOFFS', [20, 20, 5])
    assert s2a._cutoff_list(None) == [20, 5]


def test_command_line_takes_repeated_qcut(monkeypatch, tmp_path):
    monkeypatch.setattr('sys.argv', ['sam2aln', str(tmp_path / 'r.csv'), str(tmp_path / 'a.csv'),
                                     '--qcut', '0', '--qcut', '10'])
    (tmp_path / 'r.csv').write_text('')
    args = s2a.parseArgs()
    assert args.qcut == [0, 10]
    monkeypatch.setattr('sys.argv', ['sam2aln', str(tmp_path / 'r.csv'), str(tmp_path / 'a.csv')])
    assert s2a.parseArgs().qcut is None      # the module constant decides
    for h in (args.remap_csv, args.aligned_csv):
        h.close()


# ---- the (ch, thr) form of merge_pairs ------------------------------------
ALWAYS = 255


def _form(c1, q1, c2, q2, past_seq1):
    """s2a_pos of mh_sam2aln.hip for a position after both reads started:
    the merged character is ch if thr > cut else 'N'."""
    if past_seq1:
        return ('-', ALWAYS) if c2 == '-' else (c2, ord(q2))
    if c1 == c2:
        return (c1, ALWAYS) if c1 == '-' else (c1, max(ord(q1), ord(q2)))
    dq = ord(q2) - ord(q1)
    if dq >= 5:
        return c2, ord(q2)
    if dq <= -5:
        return c1, ord(q1)
    return 'N', ALWAYS


QUALS = [' ', '!', '"', '#', '%', '&', "'", '(', '0', '5', '?', 'I', '~']


@pytest.mark.parametrize('past_seq1', [False, True])
def test_cutoff_free_form_is_merge_pairs_at_every_cutoff(past_seq1):
    """Every class of position (agree, disagree by less / more than 5 either
    way, a gap in either mate with the ' ' of a deletion or the '!' of
    padding, past the shorter mate) at every cutoff 0..93."""
    checked = 0
    for c1 in 'A-':
        for c2 in 'AC-':
            for q1 in QUALS:
                for q2 in QUALS:
                    ch, thr = _form(c1, q1, c2, q2, past_seq1)
                    for cut in range(94):
                        if past_seq1:
                            got = og_sam2aln.merge_pairs('A', 'A' + c2, 'I', 'I' + q2, q_cutoff=cut)
                        else:
                            got = og_sam2aln.merge_pairs('A' + c1, 'A' + c2, 'I' + q1, 'I' + q2,
                                                         q_cutoff=cut)
                        want = ch if thr > cut + 33 else 'N'
                        assert got[1] == want, (c1, q1, c2, q2, cut, got)
                        checked += 1
                        # a gap with the quality apply_cigar (' ') or the padding
                        # ('!') gives it never wins a cutoff-dependent position;
                        # one the read itself holds, with its own quality, can
                        if got[1] == '-' and thr != ALWAYS:
                            assert (q1 if ch == c1 else q2) not in ' !'
    assert checked == 2 * 3 * len(QUALS) ** 2 * 94

"""The C-ABI library builds for gfx950, loads, and exports every entry point
include/micall_hip.h declares (no compute calls: runs without a GPU)."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    with open(os.path.join(REPO, 'include', 'micall_hip.h')) as f:
        text = f.read()
    return sorted(set(re.findall(r'^int (mh_\w+)\(', text, re.M)))


@pytest.fixture(scope='module')
def native():
    so = os.path.join(REPO, 'micall-lite_amd', 'micall_amd', 'libmicall_hip.so')
    if not os.path.exists(so):
        subprocess.run(['make', '-s', '-j8', '-C', os.path.join(REPO, 'micall-lite_amd', 'csrc')],
                       check=True)
    from micall_amd import _native
    return _native


def test_every_declared_symbol_is_exported(native):
    L = native.lib()
    names = _declared()
    assert len(names) >= 25
    for name in names:
        assert hasattr(L, name), name
    # and the binding declares a signature for every one of them
    assert set(names) <= set(native.EXPORTED)


def test_version_and_errors(native):
    assert native.lib().mh_version() == 1
    assert native.levenshtein('kitten', 'sitting') == 3


def test_pileup_info_constants_without_context(native):
    """mh_test_pileup_info with no context: the pileup's constants alone
    (what tests/pileup_path_cases.py sizes its cases by), no launch shape."""
    info = native.pileup_info()
    assert set(info) == set(native.PILEUP_INFO_FIELDS) | {'win_len'}
    assert info['max_ops'] == 128 and info['max_ins'] == 2 * info['max_ops']
    assert info['xch_span'] % 64 == 0 and info['xch_span'] > 0
    # a pair of 1024-base reads always fits
    assert info['ins_buf'] >= 3 * 1024
    assert info['tok_lds_slots'] > 0 and info['tok_lds_keys'] > 0 and info['pileup_slack'] > 0
    assert all(info[k] == 0 for k in native.PILEUP_INFO_FIELDS[7:])
    assert info['win_len'] == []
    with pytest.raises(native.NativeError):
        native.check(native.lib().mh_test_pileup_info(None, None, 0, None), 'mh_test_pileup_info')


def test_sam2aln_info_constants_without_context(native):
    """mh_test_sam2aln_info with no context: the constants that size
    k_s2a_merge's launch (what tests/s2a_merge_cases.py sizes its cases by),
    no launch shape; mh_test_set_sam2aln needs a context."""
    info = native.sam2aln_info()
    assert list(info) == list(native.SAM2ALN_INFO_FIELDS) and len(info) == 16
    # 160 KiB of LDS, four waves a block while they fit
    assert info['lds_bytes'] == 160 * 1024 and info['wpb_max'] == 4
    assert info['block_cap'] == 256 * 64 and info['min_table'] == 1024
    assert info['max_cuts'] == 8
    # c0 q0 c1 q1 per position; reference and read offset (int32) per op and mate
    assert info['span_bytes'] == 4 and info['op_bytes'] == 2 * 2 * 4
    assert all(info[k] == 0 for k in native.SAM2ALN_INFO_FIELDS[7:])
    with pytest.raises(native.NativeError):
        native.check(native.lib().mh_test_sam2aln_info(None, None), 'mh_test_sam2aln_info')
    for bits, blocks in ((64, 0), (8, 1)):
        with pytest.raises(native.NativeError, match='mh_test_set_sam2aln'):
            native.check(native.lib().mh_test_set_sam2aln(None, bits, blocks), 'mh_test_set_sam2aln')


def test_no_cpu_fallback_without_gpu(native):
    """On a host without a GPU the context refuses to start (no fallback)."""
    if native.device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(native.NativeUnavailable):
        native.Context(0)


def test_levenshtein_bit_parallel_matches_dp(native):
    """mh_levenshtein (bit-vector, 64-row blocks) against the oracle's
    cell-by-cell DP, across block boundaries and with the consensus alphabet."""
    import random

    import oracle
    rng = random.Random(7)
    alphabet = 'ACGTN-'
    lengths = [0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 701]
    for la in lengths:
        for lb in (0, 1, 64, 65, la, la + 3, max(la - 5, 0), 500):
            a = ''.join(rng.choice(alphabet) for _ in range(la))
            # b: a mutated copy half the time (small distances), random otherwise
            if rng.random() < 0.5 and la:
                b = list(a)
                for _ in range(rng.randint(0, 8)):
                    op, p = rng.randint(0, 2), rng.randrange(len(b) + 1)
                    if op == 0 and p < len(b):
                        b[p] = rng.choice(alphabet)
                    elif op == 1:
                        b.insert(p, rng.choice(alphabet))
                    elif b and p < len(b):
                        del b[p]
                b = ''.join(b)
            else:
                b = ''.join(rng.choice(alphabet) for _ in range(lb))
            assert native.levenshtein(a, b) == oracle.levenshtein(a, b), (la, len(b))
            assert native.levenshtein(b, a) == oracle.levenshtein(a, b), (la, len(b))


def test_levenshtein_batch_keeps_pair_order():
    """mh_levenshtein_batch runs its pairs longest first over host threads;
    each result still lands at its pair's index, and characters of b that a
    does not hold (mapped to one no-match symbol) count as mismatches."""
    import random

    from micall_amd import _native
    rng = random.Random(11)
    pairs = []
    for _ in range(40):
        la, lb = rng.randint(0, 400), rng.randint(0, 400)
        pairs.append((''.join(rng.choice('ACGT') for _ in range(la)),
                      ''.join(rng.choice('ACGTNxyz-') for _ in range(lb))))
    got = _native.levenshtein_many(pairs)
    assert got == [_native.levenshtein(a, b) for a, b in pairs]
    import oracle
    assert got[:8] == [oracle.levenshtein(a, b) for a, b in pairs[:8]]


def test_crc32_combine_matches_zlib(native):
    """mh_crc32_combine (the CRC-32 of A ++ B from crc(A), crc(B), |B|; the
    shift by |B| bytes as products of precomputed x^(2^k) mod P) equals
    zlib.crc32 of the concatenation, empty and odd lengths included."""
    import random
    import zlib
    rng = random.Random(5)
    for _ in range(300):
        a = rng.randbytes(rng.randint(0, 3000))
        b = rng.randbytes(rng.choice([0, 1, 2, 7, 8, 100, 4095, 70000]))
        got = native.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b))
        assert got == zlib.crc32(a + b)

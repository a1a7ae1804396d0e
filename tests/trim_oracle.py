"""
tests/trim_oracle.py -- TEST INFRASTRUCTURE ONLY.

Plain-Python statement of the 3' adapter trimming rules of
micall_amd.trim_fastqs (k_trim, csrc/mh_censor.hip),
used to check the device on small inputs.  It is pinned by a brute-force
edit distance in tests/test_trim_oracle.py.

For an adapter a (length m) and a read r (length n, the sequence line as the
censor pass left it), c(i, j) is the smallest unit-cost edit distance between
a[:i] and any r[s:j], and s(i, j) the smallest s that attains it.  Bytes are
compared for equality, so an 'N' in the read matches nothing.

Candidates: (m, j) for every j with c <= E[m] (the whole adapter anywhere),
and (i, n) for min_overlap <= i < m with c <= E[i] (a prefix of the adapter at
the read's end).  Over every adapter of the record's list the candidate with
the smallest s wins; ties go to the smaller cost, then the larger i, then the
lower adapter index.  The read and its quality line are cut to s.
"""
import gzip

import numpy as np

MAX_ADAPTERS = 8
MIN_ADAPTER, MAX_ADAPTER = 3, 64
MAX_READ = 65535


def error_table(error_rate):
    """E[i] = int(i * error_rate), i = 0..64."""
    return [int(i * error_rate) for i in range(MAX_ADAPTER + 1)]


def check_args(adapters1, adapters2, min_overlap, max_errors):
    for adapters in (adapters1, adapters2):
        if len(adapters) > MAX_ADAPTERS:
            raise ValueError('more than {} adapters'.format(MAX_ADAPTERS))
        for a in adapters:
            if not MIN_ADAPTER <= len(a) <= MAX_ADAPTER or set(a) - set('ACGT'):
                raise ValueError('bad adapter {!r}'.format(a))
    if min_overlap < 1:
        raise ValueError('min_overlap below 1')
    if len(max_errors) != MAX_ADAPTER + 1 or any(not 0 <= e < max(i, 1) for i, e in enumerate(max_errors)):
        raise ValueError('bad error table')


def table(a, r):
    """K[i][j] = c(i, j) << 16 | s(i, j) by the packed recurrence."""
    m, n = len(a), len(r)
    K = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(n + 1):
        K[0][j] = j
    for i in range(1, m + 1):
        K[i][0] = i << 16
        for j in range(1, n + 1):
            K[i][j] = min(K[i - 1][j - 1] + ((a[i - 1] != r[j - 1]) << 16),
                          K[i - 1][j] + (1 << 16),
                          K[i][j - 1] + (1 << 16))
    return K


def cost_origin(a, r):
    """[[(c(i, j), s(i, j)) for j in 0..n] for i in 0..m]"""
    return [[(k >> 16, k & 0xffff) for k in row] for row in table(a, r)]


def table_rows(a, r):
    """table(a, r) as an (m + 1, n + 1) array, a row at a time: with
    D[j] = min(diagonal, up) and D[0] = K[i][0], the left term makes
    K[i][j] = min over j' <= j of D[j'] + ((j - j') << 16), a running
    minimum.  Only a faster way to the same numbers (the fuzz files hold
    millions of cells); tests/test_trim_oracle.py holds it to table()."""
    m, n = len(a), len(r)
    rb = np.frombuffer(r.encode('latin-1'), dtype=np.uint8)
    step = np.arange(n + 1, dtype=np.int64) << 16
    K = np.empty((m + 1, n + 1), dtype=np.int64)
    K[0] = np.arange(n + 1)
    for i in range(1, m + 1):
        D = np.empty(n + 1, dtype=np.int64)
        D[0] = i << 16
        D[1:] = np.minimum(K[i - 1, :-1] + ((rb != ord(a[i - 1])).astype(np.int64) << 16),
                           K[i - 1, 1:] + (1 << 16))
        K[i] = np.minimum.accumulate(D - step) + step
    return K


def best(r, adapters, min_overlap, max_errors):
    """The winning candidate of read r over the adapters as (s, cost, i,
    adapter index), or None."""
    n = len(r)
    if n > MAX_READ:
        raise ValueError('read longer than {} bases'.format(MAX_READ))
    win = None
    for idx, a in enumerate(adapters):
        m = len(a)
        K = table_rows(a, r)
        # full candidates: every column of row m within E[m]
        cands = [(m, int(k)) for k in K[m][(K[m] >> 16) <= max_errors[m]]]
        # partial candidates: column n of the rows min_overlap .. m - 1
        cands += [(i, int(K[i, n])) for i in range(min_overlap, m)
                  if (K[i, n] >> 16) <= max_errors[i]]
        for i, k in cands:
            key = (k & 0xffff, k >> 16, -i, idx)
            if win is None or key < win:
                win = key
    if win is None:
        return None
    return win[0], win[1], -win[2], win[3]


def trim_bytes(data, adapters1, adapters2, min_overlap, max_errors, use_gzip=False, classes=None):
    """(trimmed FASTQ bytes, stats) for censored FASTQ bytes (the output of
    og_censor.censor_bytes): stats[(direction, adapter index)] = [reads,
    bases] with direction 1 for records whose header says read 1, else 2.
    classes, a dict, gets the number of records whose winner is a 'full' or a
    'partial' candidate and of the 'untrimmed' ones."""
    check_args(adapters1, adapters2, min_overlap, max_errors)
    if use_gzip:
        data = gzip.decompress(data)
    lines = data.split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0
    lines.pop()
    out, stats = [], {}
    for k in range(0, len(lines), 4):
        ident, seq, opt, qual = lines[k:k + 4]
        second = (ident.decode() + '\n').split(' ')[1]     # the line with its newline, as censor
        direction = 1 if second.split(':')[0] == '1' else 2
        adapters = adapters1 if direction == 1 else adapters2
        win = best(seq.decode('latin-1'), adapters, min_overlap, max_errors)
        if classes is not None:
            kind = 'untrimmed' if win is None else 'full' if win[2] == len(adapters[win[3]]) else 'partial'
            classes[kind] = classes.get(kind, 0) + 1
        if win is not None:
            s, _, _, idx = win
            st = stats.setdefault((direction, idx), [0, 0])
            st[0] += 1
            st[1] += len(seq) - s
            seq, qual = seq[:s], qual[:s]
        out += [ident, seq, opt, qual]
    return b''.join(ln + b'\n' for ln in out), stats

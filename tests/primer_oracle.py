"""
tests/primer_oracle.py -- TEST INFRASTRUCTURE ONLY.

Plain-Python statement of the anchored 5' primer trimming rules of
micall_amd.trim_fastqs (k_primer, csrc/mh_censor.hip),
used to check the device on small inputs.  It is pinned by a brute-force
edit distance in tests/test_primer_oracle.py.

For a primer p (length m) and a read r (length n, the sequence line as the
censor pass and, if adapters are set, the adapter pass left it), D(j) is the
unit-cost edit distance (substitution, insertion, deletion) between all of p
and the prefix r[0:j], for j in 0 ..= min(n, m + E[m]).  Bytes are compared
for equality, so an 'N' or a lower-case letter in the read matches nothing.

(k, j) is a candidate iff D(j) <= E[m].  Over the primers of the record's list
the candidates are ordered by: the larger m - D, then the smaller D, then the
larger j, then the lower primer index k.  With no candidate the record is
unchanged; otherwise lead = j, the sequence line is written as seq[lead:] and
the quality line as qual[min(lead, len(qual)):].
"""
import gzip

import numpy as np

MAX_PRIMERS = 256
MIN_PRIMER, MAX_PRIMER = 8, 64
MAX_COLUMN = 127


def error_table(error_rate):
    """E[i] = int(i * error_rate), i = 0..64."""
    return [int(i * error_rate) for i in range(MAX_PRIMER + 1)]


def check_args(primers1, primers2, max_errors):
    for primers in (primers1, primers2):
        if len(primers) > MAX_PRIMERS:
            raise ValueError('more than {} primers'.format(MAX_PRIMERS))
        for p in primers:
            if not MIN_PRIMER <= len(p) <= MAX_PRIMER or set(p) - set('ACGT'):
                raise ValueError('bad primer {!r}'.format(p))
    if len(max_errors) != MAX_PRIMER + 1 or any(not 0 <= e < max(i, 1) or i + e > MAX_COLUMN
                                                for i, e in enumerate(max_errors)):
        raise ValueError('bad error table')


def distances(p, r, max_err):
    """[D(j) for j in 0 ..= min(n, m + max_err)] by the cell recurrence
    D[i][j] = min(D[i-1][j-1] + (p[i-1] != r[j-1]), D[i-1][j] + 1,
    D[i][j-1] + 1), D[0][j] = j, D[i][0] = i."""
    m = len(p)
    cols = min(len(r), m + max_err)
    row = list(range(cols + 1))
    for i in range(1, m + 1):
        new = [i]
        for j in range(1, cols + 1):
            new.append(min(row[j - 1] + (p[i - 1] != r[j - 1]), row[j] + 1, new[j - 1] + 1))
        row = new
    return row


def distances_many(primers, r, max_errors):
    """[distances(p, r, max_errors[len(p)]) for p in primers], every primer a
    row of one array and a DP row at a time: with T[j] = min(diagonal, up)
    and T[0] = i, the left term makes D[i][j] = min over j' <= j of T[j'] +
    (j - j'), a running minimum.  Only a faster way to the same numbers (the
    fuzz file is 4000 reads against 96 primers); tests/test_primer_oracle.py
    holds it to distances()."""
    if not primers:
        return []
    lens = np.array([len(p) for p in primers])
    cols = np.minimum(len(r), lens + np.array([max_errors[m] for m in lens]))
    width = int(cols.max())
    pb = np.zeros((len(primers), int(lens.max())), dtype=np.uint8)
    for k, p in enumerate(primers):
        pb[k, :len(p)] = np.frombuffer(p.encode('latin-1'), dtype=np.uint8)
    rb = np.frombuffer(r[:width].encode('latin-1'), dtype=np.uint8)
    step = np.arange(width + 1, dtype=np.int16)
    prev = np.tile(step, (len(primers), 1))
    last = np.empty_like(prev)
    ends = {int(m): np.nonzero(lens == m)[0] for m in set(lens.tolist())}
    for i in range(1, pb.shape[1] + 1):
        t = np.empty_like(prev)
        t[:, 0] = i
        t[:, 1:] = np.minimum(prev[:, :-1] + (pb[:, i - 1, None] != rb[None, :]), prev[:, 1:] + np.int16(1))
        prev = np.minimum.accumulate(t - step, axis=1) + step
        if i in ends:
            last[ends[i]] = prev[ends[i]]
    return [last[k, :cols[k] + 1].tolist() for k in range(len(primers))]


def best(r, primers, max_errors):
    """The winning candidate of read r over the primers as (lead, cost,
    primer index), or None."""
    win = None
    for k, row in enumerate(distances_many(primers, r, max_errors)):
        m = len(primers[k])
        if min(row) > max_errors[m]:
            continue
        for j, d in enumerate(row):
            if d <= max_errors[m]:
                key = (-(m - d), d, -j, k)
                if win is None or key < win:
                    win = key
    if win is None:
        return None
    return -win[2], win[1], win[3]


def trim_bytes(data, primers1, primers2, max_errors, use_gzip=False, classes=None):
    """(trimmed FASTQ bytes, stats) for FASTQ bytes as the passes before left
    them (the output of og_censor.censor_bytes, or of trim_oracle.trim_bytes
    after it): stats[(direction, primer index)] = [reads, bases] with
    direction 1 for records whose header says read 1, else 2.  classes, a
    dict, gets the number of records trimmed 'exact' (cost 0), 'errors'
    (cost > 0) and 'untrimmed'."""
    check_args(primers1, primers2, max_errors)
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
        primers = primers1 if direction == 1 else primers2
        win = best(seq.decode('latin-1'), primers, max_errors)
        if classes is not None:
            kind = 'untrimmed' if win is None else 'exact' if win[1] == 0 else 'errors'
            classes[kind] = classes.get(kind, 0) + 1
        if win is not None:
            lead, _, idx = win
            st = stats.setdefault((direction, idx), [0, 0])
            st[0] += 1
            st[1] += lead
            seq, qual = seq[lead:], qual[min(lead, len(qual)):]
        out += [ident, seq, opt, qual]
    return b''.join(ln + b'\n' for ln in out), stats

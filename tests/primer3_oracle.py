"""
tests/primer3_oracle.py -- TEST INFRASTRUCTURE ONLY.

Plain-Python statement of the 3' primer trimming rules of
micall_amd.trim_fastqs (k_primer3, csrc/mh_censor.hip),
used to check the device on small inputs.  It is pinned by a brute-force edit
distance in tests/test_primer3_oracle.py.

The text is x = r[lead:n]: r the sequence line as the censor pass and, if
adapters are set, the adapter pass left it, n its length, lead what the 5'
primer pass decided (0 without 5' primers).  Bytes are compared for equality,
so an 'N' or a lower-case letter in the read matches nothing.  The pattern is
a 3' primer p of m bases, E the integer error table, b the number of bases
cut from the end.

Full candidates: (k, b) for 1 <= b <= len(x) with F(b) <= E[m], F(b) the
minimum over e in n-b ..= n of the unit-cost edit distance between all of p
and r[n-b:e] -- the primer, whole, starts exactly at the cut and ends
anywhere.  Partial candidates: (k, b) for min_overlap <= b <= min(len(x),
m - 1) with G(b) <= E[b], G(b) the minimum over i in 0 ..= m of the edit
distance between p[:i] and all of r[n-b:n] -- the read ends inside the primer.

Both are one DP each on the reversed strings (q = p reversed, t = x reversed,
column b = bases cut), cell recurrence
    D[i][j] = min(D[i-1][j-1] + (q[i-1] != t[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
with A[0][j] = 0, A[i][0] = i -> F(b) = A[m][b] and B[0][j] = j, B[i][0] = 0
-> G(b) = B[m][b].

With L = m for a full candidate and L = b for a partial one, the candidates
over the primers of the record's list are ordered by: the larger L - D, then
the smaller D, then the larger b, then the lower primer index k.  With no
candidate the record is unchanged; otherwise the sequence line keeps n - b
bases and the quality line at most n - b.
"""
import gzip

import numpy as np

MAX_PRIMERS = 256
MIN_PRIMER, MAX_PRIMER = 8, 64
MAX_READ = 65535


def error_table(error_rate):
    """E[i] = int(i * error_rate), i = 0..64."""
    return [int(i * error_rate) for i in range(MAX_PRIMER + 1)]


def check_args(primers1, primers2, max_errors, min_overlap):
    for primers in (primers1, primers2):
        if len(primers) > MAX_PRIMERS:
            raise ValueError('more than {} primers'.format(MAX_PRIMERS))
        for p in primers:
            if not MIN_PRIMER <= len(p) <= MAX_PRIMER or set(p) - set('ACGT'):
                raise ValueError('bad primer {!r}'.format(p))
    if len(max_errors) != MAX_PRIMER + 1 or any(not 0 <= e < max(i, 1) for i, e in enumerate(max_errors)):
        raise ValueError('bad error table')
    if int(min_overlap) != min_overlap or not 1 <= min_overlap <= MAX_PRIMER:
        raise ValueError('bad min_overlap')


def _last_row(q, t, row0, col0):
    """Row len(q) of the cell recurrence over q (rows) and t (columns) with
    D[0][j] = row0(j) and D[i][0] = col0(i)."""
    row = [row0(j) for j in range(len(t) + 1)]
    for i in range(1, len(q) + 1):
        new = [col0(i)]
        for j in range(1, len(t) + 1):
            new.append(min(row[j - 1] + (q[i - 1] != t[j - 1]), row[j] + 1, new[j - 1] + 1))
        row = new
    return row


def full_costs(p, x):
    """[F(b) for b in 0 ..= len(x)]: table A."""
    return _last_row(p[::-1], x[::-1], lambda j: 0, lambda i: i)


def partial_costs(p, x):
    """[G(b) for b in 0 ..= len(x)]: table B."""
    return _last_row(p[::-1], x[::-1], lambda j: j, lambda i: 0)


def best(r, lead, primers, max_errors, min_overlap):
    """The winning candidate of read r behind its lead over the primers as
    (b, cost, primer index, 'full' or 'partial'), or None: the rules as they
    are written above, a cell at a time."""
    x = r[lead:]
    win = None
    for k, p in enumerate(primers):
        m = len(p)
        keys = [(-(m - d), d, -b, k, 'full') for b, d in enumerate(full_costs(p, x))
                if b >= 1 and d <= max_errors[m]]
        # G(b) looks at the last b <= m - 1 bases only
        tail = x[max(0, len(x) - (m - 1)):]
        keys += [(-(b - d), d, -b, k, 'partial') for b, d in enumerate(partial_costs(p, tail))
                 if b >= min_overlap and d <= max_errors[b]]
        for key in keys:
            if win is None or key < win:
                win = key
    if win is None:
        return None
    return -win[2], win[1], win[3], win[4]


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b'ACGT'):
    _CODE[_c] = _i


def best_many(reads, leads, primers, max_errors, min_overlap):
    """[best(r, lead, primers, max_errors, min_overlap) for r, lead in
    zip(reads, leads)], every (read, primer) pair an element of one array and
    a column at a time: the columns of A and B as Myers' vertical delta words
    over the reversed primer (tests/test_primer3_oracle.py holds the word
    operations to the cell recurrences, and this function to best()).  Only
    a faster way to the same answers: the fuzz file is 4000 reads against 96
    primers."""
    if not primers or not reads:
        return [None] * len(reads)
    texts = [r[lead:].encode('latin-1')[::-1] for r, lead in zip(reads, leads)]
    lens = np.array([len(t) for t in texts])
    width = int(lens.max())
    code = np.full((len(texts), max(width, 1)), 4, dtype=np.uint8)
    for i, t in enumerate(texts):
        code[i, :len(t)] = _CODE[np.frombuffer(t, dtype=np.uint8)]
    ms = np.array([len(p) for p in primers], dtype=np.int64)
    eqtab = np.zeros((5, len(primers)), dtype=np.uint64)
    for k, p in enumerate(primers):
        for i, c in enumerate(p[::-1]):
            eqtab['ACGT'.index(c), k] |= np.uint64(1) << np.uint64(i)
    top = (np.uint64(1) << (ms - 1).astype(np.uint64))[None, :]
    full_budget = np.array([max_errors[m] for m in ms], dtype=np.int64)[None, :]
    ks = np.arange(len(primers), dtype=np.int64)[None, :]
    shape = (len(texts), len(primers))
    one, none = np.uint64(1), np.int64(1) << 62
    state = {'A': [np.full(shape, ~np.uint64(0)), np.zeros(shape, np.uint64), np.tile(ms, (len(texts), 1))],
             'B': [np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), np.zeros(shape, np.int64)]}

    def column(which, eq):
        pv, mv, score = state[which]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | ~(xh | pv)
        mh = pv & xh
        score = score + ((ph & top) != 0) - ((mh & top) != 0)
        ph = ph << one | (one if which == 'B' else np.uint64(0))
        mh = mh << one
        state[which] = [mh | ~(xv | ph), ph & xv, score]
        return score

    win = np.full(len(texts), none)
    for b in range(1, width + 1):
        eq = eqtab[code[:, b - 1]]
        live = (lens >= b)[:, None]
        d = column('A', eq)
        key = (64 - (ms[None, :] - d)) << 30 | d << 24 | (MAX_READ - b) << 8 | ks
        win = np.minimum(win, np.where(live & (d <= full_budget), key, none).min(axis=1))
        if b <= MAX_PRIMER - 1:
            d = column('B', eq)
            if b >= min_overlap:
                key = (64 - (b - d)) << 30 | d << 24 | (MAX_READ - b) << 8 | ks
                ok = live & (b < ms)[None, :] & (d <= max_errors[b])
                win = np.minimum(win, np.where(ok, key, none).min(axis=1))
    out = []
    for w in win.tolist():
        if w == none:
            out.append(None)
            continue
        k, b, d, span = w & 255, MAX_READ - (w >> 8 & 0xffff), w >> 24 & 63, 64 - (w >> 30)
        out.append((b, d, k, 'full' if span + d == len(primers[k]) else 'partial'))
    return out


def leads_of(data, primers1, primers2, max_errors):
    """The per-record leads tests/primer_oracle.py decides on FASTQ bytes as
    the censor and adapter passes left them (0 where no 5' primer matches)."""
    import primer_oracle
    lines = data.split(b'\n')
    leads = []
    for k in range(0, len(lines) - 1, 4):
        second = (lines[k].decode() + '\n').split(' ')[1]
        primers = primers1 if second.split(':')[0] == '1' else primers2
        win = primer_oracle.best(lines[k + 1].decode('latin-1'), primers, max_errors)
        leads.append(0 if win is None else win[0])
    return leads


def trim_bytes(data, leads, primers1, primers2, max_errors, min_overlap, use_gzip=False, classes=None):
    """(trimmed FASTQ bytes, stats) for FASTQ bytes as the censor and adapter
    passes left them and the per-record leads of the 5' primer pass (None:
    all 0): the sequence line is written as seq[lead:n - b], the quality line
    from min(lead, its kept length) to min(its length, n - b), as the writer
    does.  stats[(direction, primer index)] = [reads, bases] with direction 1
    for records whose header says read 1, else 2.  classes, a dict, gets the
    number of records 'full exact', 'full errors', 'partial' and
    'untrimmed'."""
    check_args(primers1, primers2, max_errors, min_overlap)
    if use_gzip:
        data = gzip.decompress(data)
    lines = data.split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0
    lines.pop()
    count = len(lines) // 4
    if leads is None:
        leads = [0] * count
    assert len(leads) == count
    directions = []
    for k in range(0, len(lines), 4):
        second = (lines[k].decode() + '\n').split(' ')[1]     # the line with its newline, as censor
        directions.append(1 if second.split(':')[0] == '1' else 2)
    wins = [None] * count
    for direction, primers in ((1, primers1), (2, primers2)):
        idx = [i for i in range(count) if directions[i] == direction]
        seqs = [lines[4 * i + 1].decode('latin-1') for i in idx]
        if any(len(s) > MAX_READ for s in seqs):
            raise ValueError('a read of more than {} bases'.format(MAX_READ))
        for i, win in zip(idx, best_many(seqs, [min(leads[i], len(s)) for i, s in zip(idx, seqs)], primers,
                                         max_errors, min_overlap)):
            wins[i] = win
    out, stats = [], {}
    for i in range(count):
        ident, seq, opt, qual = lines[4 * i:4 * i + 4]
        win = wins[i]
        if classes is not None:
            kind = 'untrimmed' if win is None else 'partial' if win[3] == 'partial' else \
                'full exact' if win[1] == 0 else 'full errors'
            classes[kind] = classes.get(kind, 0) + 1
        keep_seq, keep_qual = len(seq), len(qual)
        if win is not None:
            b, _, idx, _ = win
            st = stats.setdefault((directions[i], idx), [0, 0])
            st[0] += 1
            st[1] += b
            keep_seq -= b
            keep_qual = min(keep_qual, keep_seq)
        lead = min(leads[i], keep_seq)
        out += [ident, seq[lead:keep_seq], opt, qual[min(lead, keep_qual):keep_qual]]
    return b''.join(ln + b'\n' for ln in out), stats

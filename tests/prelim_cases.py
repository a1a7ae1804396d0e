"""prelim.csv edge texts and a Python restatement of how remap() reads the
file back (remap.py:474-498): csv.DictReader, remap.matchmaker over the rows
whose rname is an @SQ name, compact reference ids.  Shared by
test_csv_readers_host.py and test_gpu_prelim_csv.py."""
import csv
import io
import re

import numpy as np

REFNAMES = ['refA', 'refB']
HEAD = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual'
MAXOPS = 128                                   # MH_MAXOPS
OPS = {'M': 0, 'I': 1, 'D': 2, 'S': 4}         # MH_OP_*; any other letter is op 3


def row(qname, flag, rname, pos, cigar, seq, qual):
    return ','.join([qname, str(flag), rname, str(pos), '0', cigar, '=', '1', '0', seq, qual])


PLAIN_ROWS = [row('a', 99, 'refA', 1, '5M', 'ACGTA', 'IIIII'),
              row('a', 147, 'refA', 3, '5M', 'GTACC', 'IIIII'),
              row('b', 99, 'refB', 2, '2M1I2M', 'ACGTA', 'HHHHH'),
              row('b', 147, 'refB', 4, '3M1D2M', 'GTACC', 'HHH'),       # short qual: padded
              row('c', 163, 'refA', 2, '5M', 'CGTAC', 'GGGGGGG')]       # long qual: cut
PLAIN = '\n'.join([HEAD] + PLAIN_ROWS) + '\n'

# one quoted qname that holds line ends and fills the middle of the body: the
# first '\n' at or after every even split of 2 and of 3 blocks is inside it
INNER_NEWLINE = '\n'.join([HEAD, PLAIN_ROWS[0],
                           row('"q\nw' + 'x' * 600 + '\nz"', 99, 'refA', 1, '5M', 'ACGTA', 'IIIII'),
                           PLAIN_ROWS[1], PLAIN_ROWS[2]]) + '\n'

UNKNOWN = '\n'.join([HEAD, PLAIN_ROWS[0],
                     row('u', 99, 'other', 1, '5M', 'ACGTA', 'IIIII'),
                     row('s', 77, '*', 0, '*', 'ACGTA', 'IIIII'),
                     PLAIN_ROWS[1],
                     row('u', 147, 'other', 1, '5M', 'ACGTA', 'IIIII'),
                     row('s', 141, '*', 0, '*', 'GTACC', 'IIIII'),
                     PLAIN_ROWS[3]]) + '\n'

PERMUTED_HEAD = 'qual,seq,flag,extra,tlen,pnext,rnext,cigar,mapq,pos,rname,flag,qname'


def permuted(line):
    q, f, rn, p, mq, cg, rx, px, tl, s, ql = line.split(',')
    return ','.join([ql, s, '77', 'more', tl, px, rx, cg, mq, p, rn, f, q])


TEXTS = {
    'plain': PLAIN,
    'permuted': '\n'.join([PERMUTED_HEAD] + [permuted(r) for r in PLAIN_ROWS]) + '\n',
    'quoted_qual': '\n'.join([HEAD, row('a', 99, 'refA', 1, '5M', 'ACGTA', '"II,I""I"'),
                              row('a', 147, 'refA', 3, '5M', 'GTACC', '"""",,,'),
                              PLAIN_ROWS[2]]) + '\n',
    'quoted_qname': '\n'.join([HEAD, row('"a,1"', 99, 'refA', 1, '5M', 'ACGTA', 'IIIII'),
                               row('"a,1"', 147, 'refA', 3, '5M', 'GTACC', 'IIIII'),
                               row('"a""1"', 99, 'refA', 3, '5M', 'GTACC', 'IIIII'),
                               row('"a""1"', 147, 'refA', 3, '5M', 'GTACC', 'IIIII')]) + '\n',
    'inner_newline': INNER_NEWLINE,
    'after_closing_quote': '\n'.join([HEAD, row('"ab"cd', 99, 'refA', 1, '5M', 'ACGTA', 'IIIII'),
                                      row('abcd', 147, 'refA', 3, '5M', 'GTACC', '"II"III')]) + '\n',
    'crlf': PLAIN.replace('\n', '\r\n'),
    'lone_cr': '\n'.join([HEAD, PLAIN_ROWS[0] + '\r' + PLAIN_ROWS[1], PLAIN_ROWS[2]]) + '\n',
    'blank_lines': '\n'.join([HEAD, '', PLAIN_ROWS[0], '', '\r', PLAIN_ROWS[1], '']) + '\n\n',
    'no_final_newline': PLAIN[:-1],
    'unknown_rnames': UNKNOWN,
    'unpaired_mate': '\n'.join([HEAD, PLAIN_ROWS[0], PLAIN_ROWS[2], PLAIN_ROWS[3]]) + '\n',
    'three_of_one_qname': '\n'.join([HEAD, PLAIN_ROWS[0], PLAIN_ROWS[1], PLAIN_ROWS[0]]) + '\n',
    'cigars': '\n'.join([HEAD, row('a', 99, 'refA', 1, '1M' * (MAXOPS + 1), 'A' * (MAXOPS + 1), 'I'),
                         row('a', 147, 'refA', 3, '1M' * MAXOPS, 'A' * MAXOPS, 'I'),
                         row('b', 99, 'refA', 3, '5Q', 'GTACC', 'IIIII'),
                         row('b', 147, 'refA', 3, '5', 'GTACC', 'IIIII'),
                         row('c', 99, 'refA', 3, '2H3M', 'GTACC', 'IIIII'),
                         row('c', 157, 'refA', 3, 'bad', 'GTACC', 'IIIII')]) + '\n',   # flag & 4: no ops
    'header_only': HEAD + '\n',
}

ERRORS = {
    'short_row': ('\n'.join([HEAD, PLAIN_ROWS[0], 'a,147,refA,3', PLAIN_ROWS[2]]) + '\n',
                  'prelim csv: short row'),
    'missing_column': (PLAIN.replace(',cigar,', ',cigars,'), 'prelim csv: missing column cigar'),
    'empty': ('', 'prelim csv: empty'),
}


def atoi(s):
    """C atoi on the flag and pos fields (the reader is lenient on purpose)."""
    m = re.match(r'[ \t]*([+-]?)(\d*)', s)
    return int(m.group(1) + (m.group(2) or '0'))


def cigar_words(cigar):
    if not re.match(r'^((\d+)([MIDNSHPX=]))*$', cigar):
        return [3], 0
    pairs = re.findall(r'(\d+)([MIDNSHPX=])', cigar)
    maxm = max([int(n) for n, op in pairs if op == 'M'] or [0])
    if len(pairs) > MAXOPS:
        return [3], maxm
    return [(int(n) << 4) | OPS.get(op, 3) for n, op in pairs], maxm


def matchmaker(rows):
    """remap.matchmaker (remap.py:853-889) with include_singles=True over
    (index, qname) rows."""
    cached = {}
    for i, qname in rows:
        old = cached.pop(qname, None)
        if old is None:
            cached[qname] = i
        else:
            yield old, i
    for i in cached.values():
        yield i, -1


def restate(text, refnames=REFNAMES):
    """What prelim_parse returns for text: (rows_load arguments, info dict),
    every data row in file order."""
    rows = list(csv.DictReader(io.StringIO(text, newline='')))
    flag = [atoi(r['flag']) for r in rows]
    pos = [atoi(r['pos']) for r in rows]
    unknown, name_id = [], []
    for r in rows:
        if r['rname'] in refnames:
            name_id.append(refnames.index(r['rname']))
        else:
            if r['rname'] not in unknown:
                unknown.append(r['rname'])
            name_id.append(-1 - unknown.index(r['rname']))
    units = [i for pair in matchmaker((i, r['qname']) for i, r in enumerate(rows) if name_id[i] >= 0)
             for i in pair]
    present = sorted({name_id[i] for i in units if i >= 0})
    ref = [present.index(n) if n in present else 0 for n in name_id]
    cig, cig_off, n_cig, maxm = [], [], [], []
    for r, f in zip(rows, flag):
        ops, m = cigar_words(r['cigar']) if not f & 4 else ([], 0)
        cig_off.append(len(cig))
        n_cig.append(len(ops))
        maxm.append(m)
        cig += ops
    seq = ''.join(r['seq'] for r in rows).encode()
    qual = ''.join(r['qual'][:len(r['seq'])].ljust(len(r['seq']), 'J') for r in rows).encode()
    lens = [len(r['seq']) for r in rows]
    offs = [0] + np.cumsum(lens, dtype=np.int64).tolist()[:-1] if rows else []
    info = [[name_id[i], flag[i], maxm[i], ref[i]] for i in range(len(rows))]
    args = (flag, ref, pos, cig_off, n_cig, cig, seq, qual, offs, lens, units)
    return args, dict(n_rows=len(rows), n_units=len(units) // 2, info=info, present=present,
                      unknown=unknown)


def assert_same(got, want, what=''):
    """Every array of a prelim_parse result against restate()'s."""
    (gargs, ginfo), (wargs, winfo) = got, want
    names = ('flag', 'ref', 'pos', 'cig_off', 'n_cigar', 'cigar', 'seq', 'qual', 'offsets', 'lens', 'units')
    for name, g, w in zip(names, gargs, wargs):
        g = np.asarray(g)
        if name in ('seq', 'qual'):
            assert g.tobytes() == w, (what, name)
        else:
            assert g.tolist() == list(w), (what, name)
    assert ginfo['n_rows'] == winfo['n_rows'] and ginfo['n_units'] == winfo['n_units'], what
    assert np.asarray(ginfo['info']).reshape(-1, 4).tolist() == winfo['info'], (what, 'info')
    assert list(ginfo['present']) == winfo['present'], (what, 'present')
    assert list(ginfo['unknown']) == winfo['unknown'], (what, 'unknown')

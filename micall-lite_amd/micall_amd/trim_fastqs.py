"""
3' adapter trimming, anchored 5' primer trimming and 3' primer trimming of a
FASTQ file on the device, inside the censor pass:
the step the reference's chain names and does not have (bin/micall:133,
"# TODO: add cutadapt step").  A sample is trimmed before the unchanged
bin/micall runs on the result:

    python -m micall_amd.trim_fastqs R1.fastq.gz R1.trimmed.fastq.gz --adapters nextera
    python -m micall_amd.trim_fastqs R1.fastq.gz R1.trimmed.fastq.gz --primers scheme.fasta

trim() is censor_fastq.censor() with adapters set on the context for the
call (mh_censor_set_adapters): the same three paths -- whole file streamed
from file to file, through bytes, a rank's block of records in a sharded job
-- with k_trim (csrc/mh_censor.hip) run after k_censor on the text already on
the device.  No host code touches a base and there is no CPU fallback.

The rules (tests/trim_oracle.py restates them).  The read
r is the sequence line as the censor pass left it: bad cycles are 'N', the
trailing bad run is dropped, n bases.  Bytes are compared for equality, so an
'N' or a lower-case letter in the read matches nothing.  For an adapter a of
m bases, c(i, j) is the smallest unit-cost edit distance (substitution,
insertion, deletion) between a[:i] and any r[s:j], s(i, j) the smallest s
that attains it.  With E[i] = int(i * error_rate) the candidates are
  full     (m, j) for every j in 0..n with c <= E[m],
  partial  (i, n) for min_overlap <= i < m with c <= E[i];
over the adapters of the record's list (adapters1 for the records whose
header says read 1, adapters2 for all others) the smallest s wins, ties going
to the smaller cost, then the larger i, then the lower adapter index.  The
sequence and quality lines are cut to s; header and '+' lines stay verbatim.
base_count and score_sum of the summary keep the reference's meaning (every
quality character of the source).

Caps: 8 adapters per list, 3 to 64 bases of ACGT each, reads of at most
65 535 kept bases (a longer one fails the call).

5' primers (primers1 / primers2; k_primer; tests/primer_oracle.py restates
the rules).  In an amplicon library every read begins with the PCR primer
that made it, and those bases are the primer's, not the sample's.  The read r
is the sequence line as the censor pass and, if adapters are set, the adapter
pass left it, n bases.  For a primer p of m bases, D(j) is the unit-cost edit
distance between all of p and the prefix r[0:j], j = 0..min(n, m + E[m]),
with E[i] = int(i * primer_error_rate).  (k, j) is a candidate when D(j) <=
E[m]: a primer matches whole or not at all, there is no min_overlap.  Over the
primers of the record's list the larger m - D wins, then the smaller D, the
larger j, the lower primer index k.  The winner's j is the record's lead: the
sequence line is written as seq[lead:kept], the quality line as
qual[min(lead, kept):kept], so a record cut to nothing stays as an empty
record and the mates stay paired.

Caps: 256 primers per list, 8 to 64 bases of ACGT each (no IUPAC codes), whole
primers at position 0 only; the read-length cap of the adapters does not
apply.  No primer scheme is bundled: give a FASTA file, a {name: sequence}
mapping or a list of sequences.

3' primers (primers3_1 / primers3_2; k_primer3; tests/primer3_oracle.py
restates the rules).  Where the insert is shorter than the read, read 1 runs
through it into the reverse complement of the primer read 2 begins with, and
read 2 into that of read 1's.  'mates' takes those reverse complements from
this call's 5' lists (primers3_1='mates': of primers2; primers3_2='mates': of
primers1); sequences given explicitly are written as they read in the read.
Neither side defaults to the other.  The text is x = r[lead:n]: r as the
passes before left it, n its kept length, lead the 5' pass's (0 without 5'
primers).  For a 3' primer p of m bases and b bases cut from the end,
  full     1 <= b <= len(x) with F(b) <= E[m], F(b) the least edit distance
           between all of p and r[n-b:e] over e in n-b..n: the primer starts
           at the cut and ends anywhere,
  partial  primer3_min_overlap <= b <= min(len(x), m - 1) with G(b) <= E[b],
           G(b) the least edit distance between p[:i] and all of r[n-b:n] over
           i in 0..m: the read ends inside the primer;
E is error_table(primer_error_rate).  With L = m for a full and L = b for a
partial candidate the larger L - D wins, then the smaller D, the larger b,
the lower primer index, and the sequence and quality lines keep n - b.

Caps: those of the 5' primers, primer3_min_overlap from 1 to 64, and the
adapters' read-length cap applies whenever a 3' list is set.

    python -m micall_amd.trim_fastqs R1.fastq.gz R1.trimmed.fastq.gz --primers left.fasta \\
        --primers2 right.fasta --primers3 mates --primers3-2 mates
"""
import argparse
import csv
import json
import os
import sys

from . import censor_fastq, session

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'adapters.json')
MAX_ADAPTERS = 8
MIN_ADAPTER, MAX_ADAPTER = 3, 64
MAX_PRIMERS = 256
MIN_PRIMER, MAX_PRIMER = 8, 64


def adapter_sets():
    with open(DATA) as f:
        return json.load(f)


def error_table(error_rate):
    """E[i] = int(i * error_rate) for i = 0..64: the one place the rate is
    used; the library and the tests' oracle take this integer table."""
    if not 0 <= error_rate < 1:
        raise ValueError('error_rate {!r} is not in [0, 1)'.format(error_rate))
    return [int(i * error_rate) for i in range(MAX_ADAPTER + 1)]


def _one_list(spec, mate, sets):
    if isinstance(spec, str):
        if spec in sets:
            return list(sets[spec]['read{}'.format(mate)])
        spec = [spec]
    return list(spec)


def resolve_adapters(adapters1, adapters2=None):
    """(list for read 1, list for the other records) of adapter strings from
    sequences, lists of sequences or a set name of data/adapters.json;
    adapters2 defaults to adapters1 (a set name: to its read 2 list)."""
    sets = adapter_sets()
    lists = (_one_list(adapters1, 1, sets),
             _one_list(adapters1 if adapters2 is None else adapters2, 2, sets))
    for adapters in lists:
        if len(adapters) > MAX_ADAPTERS:
            raise ValueError('{} adapters in one list, at most {}'.format(len(adapters), MAX_ADAPTERS))
        for a in adapters:
            if not isinstance(a, str) or not MIN_ADAPTER <= len(a) <= MAX_ADAPTER or set(a) - set('ACGT'):
                raise ValueError('adapter {!r} is neither a set name ({}) nor {} to {} bases of ACGT'.format(
                    a, ', '.join(sorted(sets)), MIN_ADAPTER, MAX_ADAPTER))
    return lists


def read_fasta(path):
    """[(name, sequence)] of a FASTA file: the name is the header's first
    word, the sequence its lines joined; a name given twice is refused."""
    entries, seen = [], set()
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith('>'):
                name = line[1:].split()[0] if line[1:].split() else ''
                if not name or name in seen:
                    raise ValueError('{}: primer name {!r} is {}'.format(
                        path, name, 'given twice' if name else 'empty'))
                seen.add(name)
                entries.append([name, ''])
            elif line:
                if not entries:
                    raise ValueError('{}: sequence before the first header'.format(path))
                entries[-1][1] += line
    return [(name, seq) for name, seq in entries]


def _one_primer_list(spec):
    if spec is None:
        return []
    if isinstance(spec, (str, os.PathLike)):
        if not os.path.isfile(spec):
            raise ValueError('primers {!r}: no such FASTA file (sequences are given as a list)'.format(spec))
        return read_fasta(spec)
    if hasattr(spec, 'items'):
        return [(str(name), seq) for name, seq in spec.items()]
    return [('primer{}'.format(k + 1), seq) for k, seq in enumerate(spec)]


def resolve_primers(primers1, primers2=None):
    """(list for read 1, list for the other records) of (name, sequence)
    from a list of sequences (named primer1, primer2, ...), a {name:
    sequence} mapping or the path of a FASTA file; primers2 defaults to
    primers1.  At most 256 primers a list, each 8 to 64 bases of ACGT."""
    lists = (_one_primer_list(primers1), _one_primer_list(primers1 if primers2 is None else primers2))
    for primers in lists:
        if len(primers) > MAX_PRIMERS:
            raise ValueError('{} primers in one list, at most {}'.format(len(primers), MAX_PRIMERS))
        for name, p in primers:
            if not isinstance(p, str) or not MIN_PRIMER <= len(p) <= MAX_PRIMER or set(p) - set('ACGT'):
                raise ValueError('primer {} ({!r}) is not {} to {} bases of ACGT'.format(
                    name, p, MIN_PRIMER, MAX_PRIMER))
    return lists


_COMPLEMENT = str.maketrans('ACGT', 'TGCA')


def reverse_complement(seq):
    return seq.translate(_COMPLEMENT)[::-1]


def resolve_primers3(primers3_1, primers3_2, plists):
    """(list for read 1, list for the other records) of (name, sequence) of
    the 3' primers, as they read in the read.  Each side is None (no list),
    the string 'mates' -- the reverse complements of the 5' list of the other
    side (plists, as resolve_primers returned it), same order, same names --
    or what resolve_primers takes; neither side defaults to the other."""
    lists = []
    for side, spec in enumerate((primers3_1, primers3_2)):
        if isinstance(spec, str) and spec == 'mates':
            mates = plists[1 - side]
            if not mates:
                raise ValueError("primers3_{} is 'mates' and primers{} is empty".format(side + 1, 2 - side))
            lists.append([(name, reverse_complement(p)) for name, p in mates])
        else:
            # primers2=[] keeps resolve_primers from filling in the other side
            lists.append(resolve_primers(spec, [])[0])
    return tuple(lists)


def trim(src, dest, adapters1, adapters2=None, bad_cycles_reader=(), use_gzip=True, summary_file=None,
         trim_summary_file=None, error_rate=0.1, min_overlap=3, primers1=None, primers2=None,
         primer_error_rate=0.1, primer_summary_file=None, primers3_1=None, primers3_2=None,
         primer3_min_overlap=12, primer3_summary_file=None):
    """Censor src (bad_cycles_reader, as censor_fastq.censor), trim 3'
    adapters, then anchored 5' primers (primers1 / primers2, as
    resolve_primers takes them) and then 3' primers (primers3_1 / primers3_2,
    as resolve_primers3 takes them) in the same device pass, into dest; empty
    adapters with primers trim primers only.  summary_file gets the
    reference's censor summary, trim_summary_file one row per given adapter:
    direction,adapter,reads,bases, primer_summary_file and
    primer3_summary_file one row per given primer:
    direction,name,primer,reads,bases.  Returns {'reads', 'bases',
    'adapters': [the adapter rows as dicts], 'primer_reads', 'primer_bases',
    'primers': [the primer rows as dicts], 'primer3_reads', 'primer3_bases',
    'primers3': [the 3' primer rows as dicts]} (summed over the ranks of a
    sharded job)."""
    lists = resolve_adapters(adapters1, adapters2)
    if int(min_overlap) != min_overlap or min_overlap < 1:
        raise ValueError('min_overlap {!r} is not a whole number >= 1'.format(min_overlap))
    table = error_table(error_rate)
    plists = resolve_primers(primers1, primers2)
    ptable = error_table(primer_error_rate)
    with_primers = bool(plists[0] or plists[1])
    p3lists = resolve_primers3(primers3_1, primers3_2, plists)
    with_primers3 = bool(p3lists[0] or p3lists[1])
    if isinstance(primer3_min_overlap, bool) or int(primer3_min_overlap) != primer3_min_overlap or \
            not 1 <= primer3_min_overlap <= MAX_PRIMER:
        raise ValueError('primer3_min_overlap {!r} is not a whole number from 1 to {}'.format(
            primer3_min_overlap, MAX_PRIMER))
    ctx = session.context()
    preads = pbases = p3reads = p3bases = [[0] * MAX_PRIMERS] * 2
    try:
        ctx.censor_set_adapters(lists[0], lists[1], int(min_overlap), table)
        if with_primers:
            ctx.censor_set_primers([p for _, p in plists[0]], [p for _, p in plists[1]], ptable)
        if with_primers3:
            ctx.censor_set_primers3([p for _, p in p3lists[0]], [p for _, p in p3lists[1]],
                                    int(primer3_min_overlap), ptable)
        censor_fastq.censor(src, bad_cycles_reader, dest, use_gzip=use_gzip, summary_file=summary_file)
        reads, bases = ctx.censor_trim_stats()
        if with_primers:
            preads, pbases = ctx.censor_primer_stats()
        if with_primers3:
            p3reads, p3bases = ctx.censor_primer3_stats()
    finally:
        ctx.censor_clear_adapters()
        ctx.censor_clear_primers()
        ctx.censor_clear_primers3()
    sh = session.shard()
    if sh is not None:
        flat = [int(x) for x in sh.sum_i64(reads[0] + reads[1] + bases[0] + bases[1])]
        reads, bases = [flat[0:8], flat[8:16]], [flat[16:24], flat[24:32]]
        if with_primers:
            n = MAX_PRIMERS
            flat = [int(x) for x in sh.sum_i64(preads[0] + preads[1] + pbases[0] + pbases[1])]
            preads, pbases = [flat[0:n], flat[n:2 * n]], [flat[2 * n:3 * n], flat[3 * n:4 * n]]
        if with_primers3:
            n = MAX_PRIMERS
            flat = [int(x) for x in sh.sum_i64(p3reads[0] + p3reads[1] + p3bases[0] + p3bases[1])]
            p3reads, p3bases = [flat[0:n], flat[n:2 * n]], [flat[2 * n:3 * n], flat[3 * n:4 * n]]
    rows = [dict(direction=d + 1, adapter=a, reads=reads[d][k], bases=bases[d][k])
            for d in (0, 1) for k, a in enumerate(lists[d])]
    prows = [dict(direction=d + 1, name=name, primer=p, reads=preads[d][k], bases=pbases[d][k])
             for d in (0, 1) for k, (name, p) in enumerate(plists[d])]
    p3rows = [dict(direction=d + 1, name=name, primer=p, reads=p3reads[d][k], bases=p3bases[d][k])
              for d in (0, 1) for k, (name, p) in enumerate(p3lists[d])]
    if trim_summary_file is not None and session.is_writer():
        writer = csv.DictWriter(trim_summary_file, ['direction', 'adapter', 'reads', 'bases'],
                                lineterminator=os.linesep)
        writer.writeheader()
        writer.writerows(rows)
    if primer_summary_file is not None and session.is_writer():
        writer = csv.DictWriter(primer_summary_file, ['direction', 'name', 'primer', 'reads', 'bases'],
                                lineterminator=os.linesep)
        writer.writeheader()
        writer.writerows(prows)
    if primer3_summary_file is not None and session.is_writer():
        writer = csv.DictWriter(primer3_summary_file, ['direction', 'name', 'primer', 'reads', 'bases'],
                                lineterminator=os.linesep)
        writer.writeheader()
        writer.writerows(p3rows)
    return dict(reads=sum(r['reads'] for r in rows), bases=sum(r['bases'] for r in rows), adapters=rows,
                primer_reads=sum(r['reads'] for r in prows), primer_bases=sum(r['bases'] for r in prows),
                primers=prows,
                primer3_reads=sum(r['reads'] for r in p3rows), primer3_bases=sum(r['bases'] for r in p3rows),
                primers3=p3rows)


def _adapter_arg(text):
    return text if ',' not in text else [a for a in text.split(',') if a]


def _primer_arg(text):
    """--primers: a FASTA file if there is one of that name, else SEQ[,SEQ...]"""
    return text if os.path.exists(text) else [p for p in text.split(',') if p]


def _primer3_arg(text):
    """--primers3: 'mates', else as --primers"""
    return text if text == 'mates' else _primer_arg(text)


def main(argv=None):
    ap = argparse.ArgumentParser(
        prog='python -m micall_amd.trim_fastqs',
        description="Censor bad cycles and trim 3' adapters and anchored 5' primers from a FASTQ file "
                    "on the GPU.")
    ap.add_argument('src')
    ap.add_argument('dest')
    ap.add_argument('--adapters',
                    help='set name ({}) or SEQ[,SEQ...]; required unless --primers is given'.format(
                        ', '.join(sorted(adapter_sets()))))
    ap.add_argument('--adapters2', help='for the records that are not read 1 (default: --adapters)')
    ap.add_argument('--bad-cycles', help='bad_cycles.csv (tile, cycle)')
    ap.add_argument('--unzipped', action='store_true', help='src and dest are plain text, not gzip')
    ap.add_argument('--error-rate', type=float, default=0.1)
    ap.add_argument('--min-overlap', type=int, default=3)
    ap.add_argument('--summary', help='censor summary CSV (avg_quality, base_count)')
    ap.add_argument('--trim-summary', help='CSV of direction, adapter, reads, bases (default: stdout)')
    ap.add_argument('--primers', help="5' primers: FASTA file or SEQ[,SEQ...]")
    ap.add_argument('--primers2', help='for the records that are not read 1 (default: --primers)')
    ap.add_argument('--primer-error-rate', type=float, default=0.1)
    ap.add_argument('--primer-summary', help='CSV of direction, name, primer, reads, bases')
    ap.add_argument('--primers3', help="3' primers of the records of read 1, as they read in the read: "
                                       "'mates' (the reverse complements of --primers2), FASTA file or "
                                       "SEQ[,SEQ...]")
    ap.add_argument('--primers3-2', help="3' primers of the records that are not read 1 ('mates': the "
                                         "reverse complements of --primers); there is no default")
    ap.add_argument('--primer3-min-overlap', type=int, default=12)
    ap.add_argument('--primer3-summary', help="CSV of direction, name, primer, reads, bases of the 3' primers")
    args = ap.parse_args(argv)
    if args.adapters is None and args.primers is None and args.primers3 is None and args.primers3_2 is None:
        ap.error('one of --adapters, --primers and --primers3 is required')
    bad_cycles = []
    if args.bad_cycles:
        with open(args.bad_cycles) as f:
            bad_cycles = list(csv.DictReader(f))
    summary = open(args.summary, 'w') if args.summary else None
    trim_summary = open(args.trim_summary, 'w') if args.trim_summary else sys.stdout
    primer_summary = open(args.primer_summary, 'w') if args.primer_summary else None
    primer3_summary = open(args.primer3_summary, 'w') if args.primer3_summary else None
    try:
        with open(args.src, 'rb') as src, open(args.dest, 'wb') as dest:
            trim(src, dest, () if args.adapters is None else _adapter_arg(args.adapters),
                 None if args.adapters2 is None else _adapter_arg(args.adapters2),
                 bad_cycles, use_gzip=not args.unzipped, summary_file=summary,
                 trim_summary_file=trim_summary, error_rate=args.error_rate,
                 min_overlap=args.min_overlap,
                 primers1=None if args.primers is None else _primer_arg(args.primers),
                 primers2=None if args.primers2 is None else _primer_arg(args.primers2),
                 primer_error_rate=args.primer_error_rate, primer_summary_file=primer_summary,
                 primers3_1=None if args.primers3 is None else _primer3_arg(args.primers3),
                 primers3_2=None if args.primers3_2 is None else _primer3_arg(args.primers3_2),
                 primer3_min_overlap=args.primer3_min_overlap, primer3_summary_file=primer3_summary)
    finally:
        if primer3_summary is not None:
            primer3_summary.close()
        if summary is not None:
            summary.close()
        if primer_summary is not None:
            primer_summary.close()
        if trim_summary is not sys.stdout:
            trim_summary.close()


if __name__ == '__main__':
    main()

"""
3' adapter trimming of a FASTQ file on the device, inside the censor pass:
the step the reference's chain names and does not have (bin/micall:133,
"# TODO: add cutadapt step").  A sample is trimmed before the unchanged
bin/micall runs on the result:

    python -m micall_amd.trim_fastqs R1.fastq.gz R1.trimmed.fastq.gz --adapters nextera

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
65 535 kept bases (a longer one fails the call), 3' adapters only.
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


def trim(src, dest, adapters1, adapters2=None, bad_cycles_reader=(), use_gzip=True, summary_file=None,
         trim_summary_file=None, error_rate=0.1, min_overlap=3):
    """Censor src (bad_cycles_reader, as censor_fastq.censor) and trim 3'
    adapters in the same device pass, into dest.  summary_file gets the
    reference's censor summary, trim_summary_file one row per given adapter:
    direction,adapter,reads,bases.  Returns {'reads', 'bases', 'adapters':
    [those rows as dicts]} (summed over the ranks of a sharded job)."""
    lists = resolve_adapters(adapters1, adapters2)
    if int(min_overlap) != min_overlap or min_overlap < 1:
        raise ValueError('min_overlap {!r} is not a whole number >= 1'.format(min_overlap))
    table = error_table(error_rate)
    ctx = session.context()
    ctx.censor_set_adapters(lists[0], lists[1], int(min_overlap), table)
    try:
        censor_fastq.censor(src, bad_cycles_reader, dest, use_gzip=use_gzip, summary_file=summary_file)
        reads, bases = ctx.censor_trim_stats()
    finally:
        ctx.censor_clear_adapters()
    sh = session.shard()
    if sh is not None:
        flat = [int(x) for x in sh.sum_i64(reads[0] + reads[1] + bases[0] + bases[1])]
        reads, bases = [flat[0:8], flat[8:16]], [flat[16:24], flat[24:32]]
    rows = [dict(direction=d + 1, adapter=a, reads=reads[d][k], bases=bases[d][k])
            for d in (0, 1) for k, a in enumerate(lists[d])]
    if trim_summary_file is not None and session.is_writer():
        writer = csv.DictWriter(trim_summary_file, ['direction', 'adapter', 'reads', 'bases'],
                                lineterminator=os.linesep)
        writer.writeheader()
        writer.writerows(rows)
    return dict(reads=sum(r['reads'] for r in rows), bases=sum(r['bases'] for r in rows), adapters=rows)


def _adapter_arg(text):
    return text if ',' not in text else [a for a in text.split(',') if a]


def main(argv=None):
    ap = argparse.ArgumentParser(
        prog='python -m micall_amd.trim_fastqs',
        description="Censor bad cycles and trim 3' adapters from a FASTQ file on the GPU.")
    ap.add_argument('src')
    ap.add_argument('dest')
    ap.add_argument('--adapters', required=True,
                    help='set name ({}) or SEQ[,SEQ...]'.format(', '.join(sorted(adapter_sets()))))
    ap.add_argument('--adapters2', help='for the records that are not read 1 (default: --adapters)')
    ap.add_argument('--bad-cycles', help='bad_cycles.csv (tile, cycle)')
    ap.add_argument('--unzipped', action='store_true', help='src and dest are plain text, not gzip')
    ap.add_argument('--error-rate', type=float, default=0.1)
    ap.add_argument('--min-overlap', type=int, default=3)
    ap.add_argument('--summary', help='censor summary CSV (avg_quality, base_count)')
    ap.add_argument('--trim-summary', help='CSV of direction, adapter, reads, bases (default: stdout)')
    args = ap.parse_args(argv)
    bad_cycles = []
    if args.bad_cycles:
        with open(args.bad_cycles) as f:
            bad_cycles = list(csv.DictReader(f))
    summary = open(args.summary, 'w') if args.summary else None
    trim_summary = open(args.trim_summary, 'w') if args.trim_summary else sys.stdout
    try:
        with open(args.src, 'rb') as src, open(args.dest, 'wb') as dest:
            trim(src, dest, _adapter_arg(args.adapters),
                 None if args.adapters2 is None else _adapter_arg(args.adapters2),
                 bad_cycles, use_gzip=not args.unzipped, summary_file=summary,
                 trim_summary_file=trim_summary, error_rate=args.error_rate,
                 min_overlap=args.min_overlap)
    finally:
        if summary is not None:
            summary.close()
        if trim_summary is not sys.stdout:
            trim_summary.close()


if __name__ == '__main__':
    main()

"""
The nucleotide variant report in plain Python, written from its rules (the
loop of micall/core/aln2counts.py:344-375 and the writer of :537-549), and
what the variant tests share: the expected texts of the reference's twelve
variant tests (tests/golden/nuc_variants_expected.json) and a replay of their
recorded calls (tests/golden/aln2counts_golden.json) with a variant writer in
place of the recorded write_nuc_variants, which raises.
"""
import csv
import io
import json
import os
from collections import Counter

import a2c_replay

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'nuc_variants_expected.json')) as _f:
    EXPECTED = json.load(_f)
SCRIPTS = {s['test']: s for s in a2c_replay.scripts() if s['test'] in EXPECTED}
COLUMNS = ['seed', 'qcut', 'region', 'index', 'count', 'seq']


def variant_window(conseq_index):
    """(start, end) from the consensus codon of every coordinate position
    (-1: none): first = the first one, else 0; last = the last one, and -1 if
    there is none or it is 0; start = 3 first, end = 3 (last + 1)."""
    placed = [k for k in conseq_index if k >= 0]
    first = placed[0] if placed else 0
    last = placed[-1] if placed else -1
    if last == 0:
        last = -1
    return 3 * first, 3 * (last + 1)


def expected_variants(rows, start, end, ref_len, max_variants):
    """[(count, clipped)] of rows (dicts with seq, offset, count): clipped =
    ('-' * offset + seq)[start:end] counts iff twice its bytes other than '-'
    exceed ref_len; equal strings add up; sorted by (count, clipped)
    descending, the first max_variants kept."""
    counts = Counter()
    for row in rows:
        clipped = ('-' * int(row['offset']) + row['seq'])[start:end]
        if 2 * (len(clipped) - clipped.count('-')) > ref_len:
            counts[clipped] += int(row['count'])
    ranked = sorted(((n, s.encode()) for s, n in counts.items()), reverse=True)
    return [(n, s.decode()) for n, s in ranked[:max_variants]]


def tie_at_cut(rows, start, end, ref_len, max_variants):
    """Whether the cut of expected_variants leaves out a string that shares
    the last kept count."""
    more = expected_variants(rows, start, end, ref_len, max_variants + 1)
    return len(more) > max_variants > 0 and more[-1][0] == more[-2][0]


def max_variants_of(config, region):
    """getMaxVariants on a projects file in the reference's format."""
    most = 0
    for project in config['projects'].values():
        for entry in project['regions']:
            if entry['coordinate_region'] == region:
                most = max(project['max_variants'], most)
    return most


def variant_rows(seed, qcut, variants, eol=os.linesep):
    """The report's text for {region: [(count, seq)]}."""
    out = io.StringIO()
    w = csv.writer(out, lineterminator=eol)
    for name in sorted(variants):
        for i, (count, seq) in enumerate(variants[name]):
            w.writerow([seed, qcut, name, i, count, seq])
    return out.getvalue()


def oracle_write(report, handle, rows, config):
    """write_variants for oracle/og_aln2counts.py's Report: the window rule
    and expected_variants over the regions a reading frame aligned to."""
    variants = {}
    for name, mapped in report.reports.items():
        if not mapped:
            continue
        index = [-1 if t.consensus_index is None else t.consensus_index for t, _ in mapped]
        start, end = variant_window(index)
        variants[name] = expected_variants(rows, start, end, len(report.coordinate_refs[name]),
                                           max_variants_of(config, name))
    handle.write(variant_rows(report.seed, report.qcut, variants))


def replay(test, impl, write):
    """The recorded calls of one of the twelve tests against impl (as
    a2c_replay.replay takes it), write(report, handle, rows, config) called
    where the reference called write_nuc_variants: the report file's text."""
    objs, out = {}, io.StringIO()
    report_cls = a2c_replay._stubbed(impl['SequenceReport'])
    rows = config = None
    for c in SCRIPTS[test]['calls']:
        op = c['op']
        if op == 'InsertionWriter':
            objs[c['obj']] = impl['InsertionWriter'](io.StringIO())
        elif op == 'SequenceReport':
            objs[c['obj']] = report_cls(objs[c['writer']], None, c['cutoffs'])
        elif op == 'read':
            rows, config = c['rows'], c['config']
            obj = objs[c['obj']]
            obj.projects = impl['projects'](config)
            obj.overrides = {(a, b): tuple(v) for a, b, v in c['overrides']}
            obj.read(rows)
        elif op == 'write_nuc_variants_header':
            objs[c['obj']].write_nuc_variants_header(out)
        elif op == 'write_nuc_variants':
            write(objs[c['obj']], out, rows, config)
        else:
            raise AssertionError('unexpected call {} in {}'.format(op, test))
    return out.getvalue()

"""profiles/diag/covar_stage.py -- what covariation.csv costs aln2counts, by
link_stage.py's method, on the aligned.csv of one C2 pass (1M synthetic 2x251
pairs: one remap pass, then this tree's sam2aln), file to file:

    parent       aln2counts() of a built checkout of the parent commit
    plain        aln2counts() of this tree without covariation_csv (must not have changed)
    covariation  aln2counts() of this tree with covariation_csv at the thresholds below

Synthetic reads carry few real variants, so the thresholds are set to let
every called character through (min_fraction 1e-6, min_count 1): the cap of
256 variants fills and the device call has its 512 columns, the worst case.

Each runs in a process of its own (its own library and context), warmed up
twice; the timed runs alternate parent, plain, covariation, `--reps` times
(>= 7).  Reported: every sample, the medians, whether plain's median lies
inside the parent's min-max, whether plain's outputs are the parent's byte for
byte; then, from profiled runs of the covariation arm, the HIP-event times of
k_a2c_count, k_a2c_gram_bits and k_a2c_gram_pairs, and the figures of one
count_covariation over the same rows (variants kept and dropped, columns,
pairs, the native stats, its wall time).

    git worktree add ../parent HEAD~1 && make -C ../parent/micall-lite_amd/csrc
    python3 profiles/diag/covar_stage.py --parent ../parent/micall-lite_amd [--pairs N] [--reps R]
"""
import argparse
import csv
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ('k_a2c_count', 'k_a2c_detail', 'k_a2c_gram_bits', 'k_a2c_gram_pairs')
OUTPUTS = ('nuc', 'amino', 'coord_ins', 'conseq')
THRESHOLDS = dict(min_fraction=1e-6, min_count=1, max_variants=256)


def worker(args):
    sys.path.insert(0, args.package)
    from micall_amd import aln2counts, session
    covariation = args.worker == 'covariation'
    names = OUTPUTS + (('covariation',) if covariation else ())

    def run():
        handles = [open(os.path.join(args.dir, '{}.{}.csv'.format(args.name, k)), 'w') for k in names]
        try:
            with open(os.path.join(args.dir, 'aligned.csv')) as aligned:
                kw = dict({'covariation_' + k: v for k, v in THRESHOLDS.items()},
                          covariation_csv=handles[4]) if covariation else {}
                aln2counts.aln2counts(aligned, *handles[:4], **kw)
        finally:
            for h in handles:
                h.close()

    ctx = session.context()
    run()
    run()
    print(json.dumps({'ready': args.name}), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == 'run':
            t0 = time.perf_counter()
            run()
            ctx.sync()
            out = {'s': time.perf_counter() - t0, 'lib_ms': ctx.a2c_timing(0)}
        elif cmd == 'profile':
            ctx.profile(True)
            run()
            out = {}
            for kernel in KERNELS:
                ms, launches = ctx.profile_get(kernel)
                out[kernel] = {'ms': round(ms, 4), 'launches': launches}
            ctx.profile(False)
        elif cmd == 'figures':
            out = figures(args, aln2counts)
        elif cmd == 'digest':
            out = {}
            for k in names:
                h = hashlib.sha256()
                with open(os.path.join(args.dir, '{}.{}.csv'.format(args.name, k)), 'rb') as f:
                    for block in iter(lambda: f.read(1 << 24), b''):
                        h.update(block)
                out[k] = h.hexdigest()
        else:
            break
        print(json.dumps(out), flush=True)


def figures(args, aln2counts):
    """The product's count_covariation of the file's one run: what it kept,
    the columns it passed, the pairs it wrote, the native stats, wall time."""
    with open(os.path.join(args.dir, 'aligned.csv')) as f:
        rows = list(csv.DictReader(f))
    assert len({(r['refname'], r['qcut']) for r in rows}) == 1
    report = aln2counts.SequenceReport(aln2counts.InsertionWriter(open(os.devnull, 'w')),
                                       aln2counts.project_config.ProjectConfig.loadDefault(),
                                       aln2counts.CONSEQ_MIXTURE_CUTOFFS)
    report.read(rows)
    t0 = time.perf_counter()
    found = report.count_covariation(**THRESHOLDS)
    wall = time.perf_counter() - t0
    with open(os.path.join(args.dir, '{}.covariation.csv'.format(args.name))) as f:
        written = sum(1 for _ in f) - 1
    return {'rows': len(rows), 'count_covariation_s': round(wall, 4), 'stats': report.covariation_stats,
            'records': len(found), 'rows_of_the_file': written}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help="micall-lite_amd directory of a built checkout of the parent commit")
    ap.add_argument('--pairs', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--worker', choices=['plain', 'covariation'], help=argparse.SUPPRESS)
    ap.add_argument('--package', help=argparse.SUPPRESS)
    ap.add_argument('--name', help=argparse.SUPPRESS)
    ap.add_argument('--dir', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent:
        ap.error('--parent is required')
    sys.path[:0] = [REPO, os.path.join(REPO, 'micall-lite_amd')]
    import bench
    from micall_amd import _native, sam2aln
    from micall_amd.pipeline import RemapPipeline
    pairs = args.pairs
    with tempfile.TemporaryDirectory(prefix='covar_stage_') as tmp:
        ctx = _native.Context(0)
        reads, quals = bench.make_reads(pairs, block=0)
        ctx.reads_load_fixed(reads, quals, True)
        del reads, quals
        ctx.set_names(['M00000:1:000000000-AAAAA:1:1101:{}:{}'.format(1000 + i // 1000000, 1000 + i % 1000000)
                       for i in range(pairs) for _ in (0, 1)])
        RemapPipeline(ctx).run(2.0 * pairs, max_iterations=1)
        with open(os.path.join(tmp, 'remap.csv'), 'w') as f:
            f.write('qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n')
            f.write(ctx.format_rows(1, 0, 2 * pairs))
        ctx.close()
        with open(os.path.join(tmp, 'remap.csv')) as remap, open(os.path.join(tmp, 'aligned.csv'), 'w') as aligned:
            sam2aln.sam2aln(remap, aligned)
        os.unlink(os.path.join(tmp, 'remap.csv'))
        with open(os.path.join(tmp, 'aligned.csv')) as f:
            rows = sum(1 for _ in f) - 1
        print('aligned.csv written: {} rows'.format(rows), file=sys.stderr, flush=True)
        here = os.path.join(REPO, 'micall-lite_amd')
        arms = [('parent', 'plain', os.path.abspath(args.parent)), ('plain', 'plain', here),
                ('covariation', 'covariation', here)]
        procs = {}
        try:
            for name, kind, package in arms:     # one after the other: each warms up alone
                p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', kind, '--package',
                                      package, '--name', name, '--dir', tmp],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
                procs[name] = p
                assert json.loads(p.stdout.readline())['ready'] == name
                print('ready: ' + name, file=sys.stderr, flush=True)

            def ask(name, cmd):
                procs[name].stdin.write(cmd + '\n')
                procs[name].stdin.flush()
                return json.loads(procs[name].stdout.readline())

            timed = ('parent', 'plain', 'covariation')
            samples = {name: [] for name in timed}
            lib_ms = {}
            for _ in range(max(args.reps, 7)):
                for name in timed:
                    got = ask(name, 'run')
                    samples[name].append(got['s'])
                    lib_ms[name] = got['lib_ms']
            digests = {name: ask(name, 'digest') for name in timed}
            kernels = [ask('covariation', 'profile') for _ in range(3)]
            print('timed and profiled', file=sys.stderr, flush=True)
            figs = ask('covariation', 'figures')
        finally:
            for p in procs.values():
                p.stdin.close()
                p.wait(timeout=60)
    med = {name: statistics.median(v) for name, v in samples.items()}
    lo, hi = min(samples['parent']), max(samples['parent'])
    print(json.dumps({
        'workload': 'aligned.csv ({} rows) of one remap pass over {} synthetic 2x{} pairs, aln2counts file to '
                    'file; covariation = {}'.format(rows, pairs, bench.READ_LEN, json.dumps(THRESHOLDS)),
        'reps': max(args.reps, 7),
        'samples_s': {k: [round(x, 4) for x in v] for k, v in samples.items()},
        'median_s': {k: round(v, 4) for k, v in med.items()},
        'parent_min_max_s': [round(lo, 4), round(hi, 4)],
        'plain_median_inside_parent_range': lo <= med['plain'] <= hi,
        'plain_minus_parent_median_s': round(med['plain'] - med['parent'], 4),
        'covariation_over_parent': round(med['covariation'] / med['parent'], 4),
        'lib_ms': lib_ms,               # [parse, count, inserts] of the last run
        'plain_outputs_equal_parent': all(digests['plain'][k] == digests['parent'][k] for k in OUTPUTS),
        'covariation_outputs_equal_parent': all(digests['covariation'][k] == digests['parent'][k] for k in OUTPUTS),
        'kernels_ms': kernels,          # three profiled runs
        'figures': figs,
    }))


if __name__ == '__main__':
    main()

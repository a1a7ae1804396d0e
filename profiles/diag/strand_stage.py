"""profiles/diag/strand_stage.py -- what the strand support costs sam2aln, on
the remap.csv of one C2 remap pass (1M synthetic 2x251 pairs, as
s2a_phases.py builds it), file to file:

    parent   sam2aln() of a built checkout of the parent commit
    plain    sam2aln() of this tree without the new argument (must not have changed)
    strand   sam2aln() of this tree with strand_csv

Each runs in a process of its own (its own library and context), warmed up
twice; the timed runs alternate parent, plain, strand, `--reps` times (>= 7).
Reported: every sample, the medians, whether plain's median lies inside the
parent's min-max, whether plain's outputs are the parent's byte for byte;
then, from profiled runs, the HIP-event times of k_s2a_merge, k_s2a_strand and
k_s2a_strand_scan in the same call, on the C2 file and on `--pairs` copies of
one pair (every unit's adds on the same addresses).

    git worktree add ../parent HEAD~1 && make -C ../parent/micall-lite_amd/csrc
    python3 profiles/diag/strand_stage.py --parent ../parent/micall-lite_amd [--pairs N] [--reps R]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ('k_s2a_merge', 'k_s2a_strand', 'k_s2a_strand_scan')
SIDES = ('strand',)
OUTPUTS = ('aligned', 'insert', 'failed')


def worker(args):
    sys.path.insert(0, args.package)
    from micall_amd import sam2aln, session
    strand = args.worker == 'strand'

    def run(source='remap.csv'):
        paths = [os.path.join(args.dir, '{}.{}.csv'.format(args.name, k)) for k in OUTPUTS + SIDES]
        handles = [open(p, 'w') for p in paths[:4 if strand else 3]]
        try:
            with open(os.path.join(args.dir, source)) as remap:
                kw = {'strand_csv': handles[3]} if strand else {}
                sam2aln.sam2aln(remap, *handles[:3], **kw)
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
            out = {'s': time.perf_counter() - t0, 'lib_ms': ctx.sam2aln_timing()}
        elif cmd.startswith('profile'):
            ctx.profile(True)
            run(cmd.split()[1])
            out = {}
            for kernel in KERNELS:
                ms, launches = ctx.profile_get(kernel)
                out[kernel] = {'ms': round(ms, 4), 'launches': launches}
            ctx.profile(False)
        elif cmd == 'digest':
            out = {}
            for k in OUTPUTS + (SIDES if strand else ()):
                h = hashlib.sha256()
                with open(os.path.join(args.dir, '{}.{}.csv'.format(args.name, k)), 'rb') as f:
                    for block in iter(lambda: f.read(1 << 24), b''):
                        h.update(block)
                out[k] = h.hexdigest()
        else:
            break
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help="micall-lite_amd directory of a built checkout of the parent commit")
    ap.add_argument('--pairs', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--worker', choices=['plain', 'strand'], help=argparse.SUPPRESS)
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
    from micall_amd import _native
    from micall_amd.pipeline import RemapPipeline
    pairs = args.pairs
    with tempfile.TemporaryDirectory(prefix='strand_stage_') as tmp:
        ctx = _native.Context(0)
        reads, quals = bench.make_reads(pairs, block=0)
        ctx.reads_load_fixed(reads, quals, True)
        del reads, quals
        ctx.set_names(['M00000:1:000000000-AAAAA:1:1101:{}:{}'.format(1000 + i // 1000000, 1000 + i % 1000000)
                       for i in range(pairs) for _ in (0, 1)])
        RemapPipeline(ctx).run(2.0 * pairs, max_iterations=1)
        head = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'
        with open(os.path.join(tmp, 'remap.csv'), 'w') as f:
            f.write(head)
            f.write(ctx.format_rows(1, 0, 2 * pairs))
        ctx.close()
        print('remap.csv written', file=sys.stderr, flush=True)
        # the contention worst case: one pair that shares 150..194, `pairs` times
        seq, qual = 'ACGT' * 25, 'I' * 100
        with open(os.path.join(tmp, 'same.csv'), 'w') as f:
            f.write(head)
            for i in range(pairs):
                f.write('q{0},99,amp,100,44,5S95M,=,150,0,{1},{2}\nq{0},147,amp,150,44,93M7S,=,100,0,{1},{2}\n'
                        .format(i, seq, qual))
        here = os.path.join(REPO, 'micall-lite_amd')
        arms = [('parent', 'plain', os.path.abspath(args.parent), {}), ('plain', 'plain', here, {}),
                ('strand', 'strand', here, {})]
        procs = {}
        try:
            for name, kind, package, env in arms:     # one after the other: each warms up alone
                p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', kind, '--package',
                                      package, '--name', name, '--dir', tmp], env=dict(os.environ, **env),
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
                procs[name] = p
                assert json.loads(p.stdout.readline())['ready'] == name
                print('ready: ' + name, file=sys.stderr, flush=True)

            def ask(name, cmd):
                procs[name].stdin.write(cmd + '\n')
                procs[name].stdin.flush()
                return json.loads(procs[name].stdout.readline())

            timed = ('parent', 'plain', 'strand')
            samples = {name: [] for name in timed}
            lib_ms = {}
            for _ in range(max(args.reps, 7)):
                for name in timed:
                    got = ask(name, 'run')
                    samples[name].append(got['s'])
                    lib_ms[name] = got['lib_ms']
            digests = {name: ask(name, 'digest') for name in timed}
            kernels = {}
            for source in ('remap.csv', 'same.csv'):
                kernels[source] = [ask('strand', 'profile ' + source) for _ in range(3)]
        finally:
            for p in procs.values():
                p.stdin.close()
                p.wait(timeout=60)
    med = {name: statistics.median(v) for name, v in samples.items()}
    lo, hi = min(samples['parent']), max(samples['parent'])
    print(json.dumps({
        'workload': 'remap.csv of one remap pass over {} synthetic 2x{} pairs, sam2aln file to file'.format(
            pairs, bench.READ_LEN),
        'reps': max(args.reps, 7),
        'samples_s': {k: [round(x, 4) for x in v] for k, v in samples.items()},
        'median_s': {k: round(v, 4) for k, v in med.items()},
        'parent_min_max_s': [round(lo, 4), round(hi, 4)],
        'plain_median_inside_parent_range': lo <= med['plain'] <= hi,
        'plain_minus_parent_median_s': round(med['plain'] - med['parent'], 4),
        'strand_over_parent': round(med['strand'] / med['parent'], 4),
        'lib_ms': lib_ms,               # [parse, device, format aligned / insert / failed] of the last run
        'plain_outputs_equal_parent': all(digests['plain'][k] == digests['parent'][k] for k in OUTPUTS),
        'strand_outputs_equal_parent': all(digests['strand'][k] == digests['parent'][k] for k in OUTPUTS),
        'kernels_ms': kernels,          # three profiled runs each
    }))


if __name__ == '__main__':
    main()

"""profiles/diag/trim_stage.py -- what 3' adapter trimming adds to the censor
stage, on the C2 FASTQ pair (1M synthetic 2x251 pairs, each mate one gzip
file, ~2 % bad tile-cycles as bench.py's censor leg):

    parent   censor_fastq.censor() of a built checkout of the parent commit
    censor   censor_fastq.censor() of this tree (must not have changed)
    trim     trim_fastqs.trim(..., 'nextera') of this tree

Each runs in a process of its own (its own library and context), warmed up
twice; the timed runs alternate parent, censor, trim, `--reps` times (>= 5),
one run = both mates, file to file.  Reported: every sample, the medians, the
ratios to the parent, then -- from three more runs with the context's profile
on -- the kernel times of k_censor and k_trim, and whether the three censor
outputs agree (parent == censor byte for byte; trim differs).

    git worktree add ../parent HEAD~1 && make -C ../parent/micall-lite_amd/csrc
    python3 profiles/diag/trim_stage.py --parent ../parent/micall-lite_amd [--pairs N] [--reps R]
"""
import argparse
import gzip
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def worker(args):
    sys.path.insert(0, args.package)
    from micall_amd import censor_fastq, session
    if args.worker == 'trim':
        from micall_amd import trim_fastqs
    with open(os.path.join(args.dir, 'bad_cycles.json')) as f:
        rows = json.load(f)

    def run():
        for mate in (1, 2):
            src_path = os.path.join(args.dir, 'R{}.fastq.gz'.format(mate))
            dst_path = os.path.join(args.dir, '{}.R{}.out.fastq.gz'.format(args.name, mate))
            with open(src_path, 'rb') as src, open(dst_path, 'wb') as dst:
                if args.worker == 'trim':
                    trim_fastqs.trim(src, dst, 'nextera', bad_cycles_reader=iter(rows), use_gzip=True)
                else:
                    censor_fastq.censor(src, iter(rows), dst, use_gzip=True)

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
            out = {'s': time.perf_counter() - t0, 'lib_ms_last_mate': ctx.censor_timing()}
        elif cmd == 'profile':
            ctx.profile(True)
            run()
            out = {}
            for kernel in ('k_censor', 'k_trim'):
                try:
                    ms, launches = ctx.profile_get(kernel)
                    out[kernel] = {'ms': ms, 'launches': launches}
                except Exception as e:      # the parent has no k_trim
                    out[kernel] = {'error': str(e)}
            ctx.profile(False)
        elif cmd == 'digest':
            out = {}
            for mate in (1, 2):
                h = hashlib.sha256()
                with gzip.open(os.path.join(args.dir, '{}.R{}.out.fastq.gz'.format(args.name, mate))) as f:
                    for block in iter(lambda: f.read(1 << 24), b''):
                        h.update(block)
                out['R{}'.format(mate)] = h.hexdigest()
        else:
            break
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help="micall-lite_amd directory of a built checkout of the parent commit")
    ap.add_argument('--pairs', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--worker', choices=['censor', 'trim'], help=argparse.SUPPRESS)
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
    from micall_amd import projects, synth
    pol = projects.load_default().seed_sequences()['HIV1B-pol-seed']
    d = synth.make_pairs(args.pairs, genomes={'HIV1B-pol-seed': pol}, genome_seed=bench.SEED,
                         read_seed=bench.SEED, block=0, read_len=bench.READ_LEN)
    rng = random.Random(bench.SEED)
    bad = sorted({(str(1101 + t), c) for t in range(8) for c in range(1, bench.READ_LEN + 1)
                  if rng.random() < 0.02})
    with tempfile.TemporaryDirectory(prefix='trim_stage_') as tmp:
        for mate in (1, 2):
            raw = bench._fastq_text(d['r{}'.format(mate)], d['q{}'.format(mate)], mate)
            with open(os.path.join(tmp, 'R{}.fastq.gz'.format(mate)), 'wb') as f:
                f.write(gzip.compress(raw, compresslevel=1))
            del raw
        del d
        with open(os.path.join(tmp, 'bad_cycles.json'), 'w') as f:
            json.dump([{'tile': t, 'cycle': str(c)} for t, c in bad], f)
        here = os.path.join(REPO, 'micall-lite_amd')
        arms = [('parent', 'censor', os.path.abspath(args.parent)), ('censor', 'censor', here),
                ('trim', 'trim', here)]
        procs = {}
        try:
            for name, kind, package in arms:     # one after the other: each warms up alone
                p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', kind, '--package',
                                      package, '--name', name, '--dir', tmp],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
                procs[name] = p
                assert json.loads(p.stdout.readline())['ready'] == name

            def ask(name, cmd):
                procs[name].stdin.write(cmd + '\n')
                procs[name].stdin.flush()
                return json.loads(procs[name].stdout.readline())

            samples = {name: [] for name, _, _ in arms}
            lib_ms = {}
            for _ in range(max(args.reps, 5)):
                for name, _, _ in arms:
                    got = ask(name, 'run')
                    samples[name].append(got['s'])
                    lib_ms[name] = got['lib_ms_last_mate']
            kernels = {name: [] for name in ('censor', 'trim')}
            for _ in range(3):
                for name in kernels:
                    kernels[name].append(ask(name, 'profile'))
            digests = {name: ask(name, 'digest') for name, _, _ in arms}
        finally:
            for p in procs.values():
                p.stdin.close()
                p.wait(timeout=60)
    med = {name: statistics.median(v) for name, v in samples.items()}
    print(json.dumps({
        'workload': '{} synthetic 2x{} pairs, both mates censored file to file per run'.format(
            args.pairs, bench.READ_LEN),
        'bad_cycles': len(bad), 'reps': max(args.reps, 5),
        'samples_s': {k: [round(x, 4) for x in v] for k, v in samples.items()},
        'median_s': {k: round(v, 4) for k, v in med.items()},
        'censor_over_parent': round(med['censor'] / med['parent'], 4),
        'trim_over_parent': round(med['trim'] / med['parent'], 4),
        'lib_ms_last_mate': lib_ms,     # [gunzip + split, upload + kernels + download, rewrite + gzip]
        'kernels_per_run': kernels,     # three profiled runs each (two launches a run: one per mate)
        'censor_output_equals_parent': digests['censor'] == digests['parent'],
        'trim_output_differs': digests['trim'] != digests['parent'],
    }))


if __name__ == '__main__':
    main()

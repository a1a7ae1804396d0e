"""profiles/diag/primer3_stage.py -- what 3' primer trimming adds to the
trimming stage, on the C2 FASTQ pair (1M synthetic 2x251 pairs, each mate one
gzip file, ~2 % bad tile-cycles as bench.py's censor leg):

    parent    trim_fastqs.trim(..., 'nextera', primers1=96 primers) of a built
              checkout of the parent commit
    primers   the same call of this tree (launches nothing new)
    primers3  this tree's call with primers3_1 = primers3_2 = 'mates' added

Each runs in a process of its own (its own library and context), warmed up
twice; the timed runs alternate parent, primers, primers3, `--reps` times
(>= 5), one run = both mates, file to file.  Reported: every sample, the
medians and ranges, the ratios to the parent, whether parent and primers
wrote the same bytes, then -- from five runs each on the R1 file with the
context's event profile on -- the kernel times of k_censor, k_trim, k_primer
and k_primer3 with 16, 96 and 218 primers a direction (218: the size of a
tiled whole-genome scheme).

The primers are synthetic, as in primer_stage.py: 18 to 30 bases cut from the
genome the reads were drawn from at even distances, so their reverse
complements occur inside the reads of the other strand and some are trimmed
(the share is reported); k_primer3's time depends on the read lengths and
the number of primers, not on what matches.

    git worktree add ../parent HEAD~1 && make -C ../parent/micall-lite_amd/csrc
    python3 profiles/diag/primer3_stage.py --parent ../parent/micall-lite_amd [--pairs N] [--reps R]
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
SCHEMES = (16, 96, 218)
KERNELS = ('k_censor', 'k_trim', 'k_primer', 'k_primer3')


def worker(args):
    sys.path.insert(0, args.package)
    from micall_amd import session, trim_fastqs
    with open(os.path.join(args.dir, 'job.json')) as f:
        job = json.load(f)
    rows = job['bad_cycles']
    last = {}

    def run(primers, mates=(1, 2), three=False):
        last['primer_reads'] = last['primer3_reads'] = last['primer3_bases'] = 0
        for mate in mates:
            src_path = os.path.join(args.dir, 'R{}.fastq.gz'.format(mate))
            dst_path = os.path.join(args.dir, '{}.R{}.out.fastq.gz'.format(args.name, mate))
            kwargs = {'primers3_1': 'mates', 'primers3_2': 'mates'} if three else {}
            with open(src_path, 'rb') as src, open(dst_path, 'wb') as dst:
                result = trim_fastqs.trim(src, dst, 'nextera', bad_cycles_reader=iter(rows), use_gzip=True,
                                          primers1=primers, **kwargs)
            for key in last:
                last[key] += result.get(key, 0)

    three = args.worker == 'primers3'
    own = job['primers']['96']
    ctx = session.context()
    run(own, three=three)
    run(own, three=three)
    print(json.dumps({'ready': args.name}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if cmd[0] == 'run':
            t0 = time.perf_counter()
            run(own, three=three)
            ctx.sync()
            out = dict(last, s=time.perf_counter() - t0, lib_ms_last_mate=ctx.censor_timing())
        elif cmd[0] == 'profile':      # profile N: the R1 file with N primers a direction
            ctx.profile(True)
            run(job['primers'][cmd[1]], mates=(1,), three=three)
            out = {}
            for kernel in KERNELS:
                ms, launches = ctx.profile_get(kernel)
                out[kernel] = {'ms': ms, 'launches': launches}
            ctx.profile(False)
        elif cmd[0] == 'digest':
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


def spread(values):
    return {'median': round(statistics.median(values), 4), 'min': round(min(values), 4),
            'max': round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help="micall-lite_amd directory of a built checkout of the parent commit")
    ap.add_argument('--pairs', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--worker', choices=['primers', 'primers3'], help=argparse.SUPPRESS)
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
    primers = {}
    for count in SCHEMES:
        cut = []
        for k in range(count):
            at = k * (len(pol) - 30) // count
            p = pol[at:at + rng.randint(18, 30)].upper()
            cut.append(p if not set(p) - set('ACGT') else ''.join(rng.choice('ACGT') for _ in p))
        primers[str(count)] = cut
    with tempfile.TemporaryDirectory(prefix='primer3_stage_') as tmp:
        for mate in (1, 2):
            raw = bench._fastq_text(d['r{}'.format(mate)], d['q{}'.format(mate)], mate)
            with open(os.path.join(tmp, 'R{}.fastq.gz'.format(mate)), 'wb') as f:
                f.write(gzip.compress(raw, compresslevel=1))
            del raw
        del d
        with open(os.path.join(tmp, 'job.json'), 'w') as f:
            json.dump({'bad_cycles': [{'tile': t, 'cycle': str(c)} for t, c in bad], 'primers': primers}, f)
        here = os.path.join(REPO, 'micall-lite_amd')
        arms = [('parent', 'primers', os.path.abspath(args.parent)), ('primers', 'primers', here),
                ('primers3', 'primers3', here)]
        procs = {}
        try:
            print('files written', file=sys.stderr, flush=True)
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

            print('arms warmed up', file=sys.stderr, flush=True)
            samples = {name: [] for name, _, _ in arms}
            lib_ms, trimmed = {}, None
            for _ in range(max(args.reps, 5)):
                for name, _, _ in arms:
                    got = ask(name, 'run')
                    samples[name].append(got['s'])
                    lib_ms[name] = got['lib_ms_last_mate']
                    if name == 'primers3':
                        trimmed = {k: got[k] for k in ('primer_reads', 'primer3_reads', 'primer3_bases')}
                print('round done', file=sys.stderr, flush=True)
            kernels = {}
            for count in SCHEMES:
                runs = [ask('primers3', 'profile {}'.format(count)) for _ in range(5)]
                kernels[str(count)] = {k: dict(spread([r[k]['ms'] for r in runs]), launches=runs[0][k]['launches'])
                                       for k in KERNELS}
                print('profiled', count, file=sys.stderr, flush=True)
            digests = {name: ask(name, 'digest') for name, _, _ in arms}
        finally:
            for p in procs.values():
                p.stdin.close()
                p.wait(timeout=60)
    med = {name: statistics.median(v) for name, v in samples.items()}
    print(json.dumps({
        'workload': '{} synthetic 2x{} pairs, both mates trimmed file to file per run, nextera adapters and '
                    '96 5\' primers in every arm'.format(args.pairs, bench.READ_LEN),
        'bad_cycles': len(bad), 'reps': max(args.reps, 5),
        'samples_s': {k: [round(x, 4) for x in v] for k, v in samples.items()},
        'spread_s': {k: spread(v) for k, v in samples.items()},
        'primers_over_parent': round(med['primers'] / med['parent'], 4),
        'primers3_over_parent': round(med['primers3'] / med['parent'], 4),
        'lib_ms_last_mate': lib_ms,     # [gunzip + split, upload + kernels + download, rewrite + gzip]
        'trimmed_by_96_primers_per_run': trimmed,
        'kernel_ms_r1_by_primers': kernels,   # five profiled runs each: median, min, max
        'primers_output_equals_parent': digests['primers'] == digests['parent'],
        'primers3_output_differs': digests['primers3'] != digests['parent'],
    }))


if __name__ == '__main__':
    main()

"""Child process of tests/test_gpu_covariation.py: one rank of a sharded
aln2counts that writes covariation.csv, on cuda:0 (gloo: the ranks share the
test box's one GPU).  For each case directory under --cases it calls the
drop-in as bin/micall does -- every rank opens aligned.csv and the outputs --
with the thresholds of the case's covariation.json, and records how the call
ran (micall_amd.aln2counts.SHARD_STATS).  In a case named 'rank0_*' only rank
0 passes covariation_csv and the thresholds: the others must still enter the
collectives, with rank 0's thresholds."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'micall-lite_amd'))
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'covariation')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', required=True)
    args = ap.parse_args()
    from micall_amd import aln2counts as a2c
    from micall_amd import session
    sh = session.shard()
    stats = {}
    for case in sorted(os.listdir(args.cases)):
        d = os.path.join(args.cases, case)
        if not os.path.isdir(d):
            continue
        with open(os.path.join(d, 'covariation.json')) as f:
            spec = json.load(f)
        asks = sh.rank == 0 or not case.startswith('rank0_')
        handles = {k: open(os.path.join(d, k + '.csv'), 'w') for k in OUTS}
        kw = {}
        if asks:
            kw = dict(covariation_csv=handles['covariation'], covariation_min_fraction=spec['min_fraction'],
                      covariation_min_count=spec['min_count'], covariation_max_variants=spec['max_variants'])
        with open(os.path.join(d, 'aligned.csv')) as al:
            a2c.aln2counts(al, handles['nuc'], handles['amino'], handles['coord_ins'], handles['conseq'], **kw)
        for h in handles.values():
            h.close()
        stats[case] = dict(a2c.SHARD_STATS)
    with open(os.path.join(args.cases, 'rank%d.json' % sh.rank), 'w') as f:
        json.dump(stats, f)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

"""Child process of tests/test_gpu_linkage.py: one rank of a sharded aln2counts
that writes linkage.csv, on cuda:0 (gloo: the ranks share the test box's one
GPU).  For each case directory under --cases it calls the drop-in as
bin/micall does -- every rank opens aligned.csv and the outputs -- with the
positions and min_count of the case's linkage.json, and records how the call
ran (micall_amd.aln2counts.SHARD_STATS).  In a case named 'rank0_*' only rank
0 passes linkage_csv and the positions: the others must still enter the
collectives, with rank 0's sets."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'micall-lite_amd'))
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'linkage')


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
        with open(os.path.join(d, 'linkage.json')) as f:
            spec = json.load(f)
        asks = sh.rank == 0 or not case.startswith('rank0_')
        handles = {k: open(os.path.join(d, k + '.csv'), 'w') for k in OUTS}
        with open(os.path.join(d, 'aligned.csv')) as al:
            a2c.aln2counts(al, handles['nuc'], handles['amino'], handles['coord_ins'], handles['conseq'],
                           linkage_csv=handles['linkage'] if asks else None,
                           linkage_positions=spec['positions'] if asks else None,
                           linkage_min_count=spec['min_count'] if asks else 1)
        for h in handles.values():
            h.close()
        stats[case] = dict(a2c.SHARD_STATS)
    with open(os.path.join(args.cases, 'rank%d.json' % sh.rank), 'w') as f:
        json.dump(stats, f)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

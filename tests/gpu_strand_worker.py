"""Child process of tests/test_gpu_strand.py::test_two_ranks: one rank of a
sharded sam2aln with strand_csv on cuda:0 (gloo: the ranks share the test
box's one GPU).  It calls the drop-in on --dir/remap.csv as bin/micall does --
every rank opens the input and the outputs -- once with one q-cutoff ('one',
the sharded route) and once with three ('three', rank 0 alone), and records
how each call ran (micall_amd.sam2aln.SHARD_STATS)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'micall-lite_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dir', required=True)
    args = ap.parse_args()
    from micall_amd import sam2aln as s2a
    from micall_amd import session
    sh = session.shard()
    stats = {}
    for tag, cuts in (('one', [15]), ('three', [0, 10, 15])):
        names = ['{}_{}.csv'.format(tag, n) for n in ('aligned', 'insert', 'failed', 'strand')]
        handles = [open(os.path.join(args.dir, n), 'w') for n in names]
        try:
            with open(os.path.join(args.dir, 'remap.csv')) as rc:
                s2a.sam2aln(rc, *handles[:3], q_cutoffs=cuts, strand_csv=handles[3])
        finally:
            for h in handles:
                h.close()
        stats[tag] = dict(s2a.SHARD_STATS)
    with open(os.path.join(args.dir, 'rank%d.json' % sh.rank), 'w') as f:
        json.dump(stats, f)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

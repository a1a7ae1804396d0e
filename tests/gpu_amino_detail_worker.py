"""Child process of tests/test_gpu_shard_amino_detail.py: one rank of a sharded
aln2counts that writes amino_detail.csv, on cuda:0 (gloo: the ranks share the
test box's one GPU).  For each case directory under --cases it calls the
drop-in as bin/micall does -- every rank opens aligned.csv, the optional
clipping.csv and conseq_ins.csv beside it and the outputs -- and records how
the call ran (micall_amd.aln2counts.SHARD_STATS).  In a case named 'rank0_*'
only rank 0 passes amino_detail_csv: the others must still enter the sum."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'micall-lite_amd'))
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'amino_detail')


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
        asks = sh.rank == 0 or not case.startswith('rank0_')
        handles = {k: open(os.path.join(d, k + '.csv'), 'w') for k in OUTS}
        inputs = {k: open(os.path.join(d, k + '.csv')) for k in ('clipping', 'conseq_ins')
                  if os.path.exists(os.path.join(d, k + '.csv'))}
        with open(os.path.join(d, 'aligned.csv')) as al:
            a2c.aln2counts(al, handles['nuc'], handles['amino'], handles['coord_ins'], handles['conseq'],
                           clipping_csv=inputs.get('clipping'), conseq_ins_csv=inputs.get('conseq_ins'),
                           amino_detail_csv=handles['amino_detail'] if asks else None)
        for h in list(handles.values()) + list(inputs.values()):
            h.close()
        stats[case] = dict(a2c.SHARD_STATS)
    with open(os.path.join(args.cases, 'rank%d.json' % sh.rank), 'w') as f:
        json.dump(stats, f)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

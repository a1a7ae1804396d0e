"""Child process of tests/test_gpu_shard_primers3.py: one rank of a sharded
trim_fastqs.trim() with adapters, 5' primers and 3' primers ('mates') on
cuda:0 (gloo: the ranks share the test box's one GPU).  Every rank opens the
source and the destination, as bin/micall's ranks open the censor step's
files; every rank records the statistics trim() returned."""
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
    from micall_amd import session, trim_fastqs
    sh = session.shard()
    with open(os.path.join(args.dir, 'job.json')) as f:
        job = json.load(f)
    with open(os.path.join(args.dir, 'in.fastq.gz'), 'rb') as src, \
            open(os.path.join(args.dir, 'out.fastq.gz'), 'wb') as dest, \
            open(os.path.join(args.dir, 'summary.csv'), 'w') as summary, \
            open(os.path.join(args.dir, 'primer3_summary.csv'), 'w') as primer3_summary:
        result = trim_fastqs.trim(src, dest, job['adapter'], bad_cycles_reader=job['bad_cycles'],
                                  summary_file=summary, min_overlap=job['min_overlap'],
                                  primers1=job['primers1'], primers2=job['primers2'],
                                  primers3_1='mates', primers3_2='mates', primer3_summary_file=primer3_summary)
    with open(os.path.join(args.dir, 'rank%d.json' % sh.rank), 'w') as f:
        json.dump(result, f)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

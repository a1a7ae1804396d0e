"""Child process of tests/test_gpu_variants.py: one rank of a sharded
aln2counts with variants_csv, on cuda:0 (gloo: the ranks share the test
box's one GPU).  Every rank opens aligned.csv and the outputs in --dir as
bin/micall does and passes projects.json as json; rank 0 first runs the
unsharded computation into *.single files, the expectation of the test.  How
the call ran (micall_amd.aln2counts.SHARD_STATS) goes to rank<r>.json."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'micall-lite_amd'))
OUTS = ('nuc', 'amino', 'coord_ins', 'conseq', 'failed', 'coverage', 'variants')


def _run(call, d, suffix, proj):
    handles = {k: open(os.path.join(d, k + suffix), 'w') for k in OUTS}
    try:
        with open(os.path.join(d, 'aligned.csv')) as al:
            call(al, handles, proj)
    finally:
        for h in handles.values():
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dir', required=True)
    d = ap.parse_args().dir
    from micall_amd import aln2counts as a2c
    from micall_amd import session
    sh = session.shard()
    proj = os.path.join(d, 'projects.json')
    if sh.rank == 0:
        _run(lambda al, h, p: a2c._aln2counts(al, h['nuc'], h['amino'], h['coord_ins'], h['conseq'],
                                              h['failed'], None, None, h['coverage'], p,
                                              variants_csv=h['variants']), d, '.single', proj)
    _run(lambda al, h, p: a2c.aln2counts(al, h['nuc'], h['amino'], h['coord_ins'], h['conseq'],
                                         failed_align_csv=h['failed'],
                                         coverage_summary_csv=h['coverage'], json=p,
                                         variants_csv=h['variants']), d, '.csv', proj)
    with open(os.path.join(d, 'rank%d.json' % sh.rank), 'w') as f:
        json.dump(dict(a2c.SHARD_STATS), f)
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

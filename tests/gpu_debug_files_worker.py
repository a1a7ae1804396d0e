"""Child process of tests/test_gpu_sam_to_conseqs.py: one rank of a sharded
remap(debug_file_prefix=...) on cuda:0 (gloo: the ranks share the test box's
one GPU), as tests/gpu_dropin_worker.py runs the drop-ins.  Every rank opens
the same remap.csv; the debug files are opened by remap() itself."""
import gzip
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'micall-lite_amd'))


def main():
    d, out = sys.argv[1], sys.argv[2]
    from micall_amd import remap as rm
    from micall_amd import session

    r1 = os.path.join(d, 'R1.fastq.gz')
    r2 = os.path.join(d, 'R2.fastq.gz')
    r2 = r2 if os.path.exists(r2) else None
    with gzip.open(os.path.join(d, 'prelim.csv.gz'), 'rt') as f:
        prelim = io.StringIO(f.read())
    with open(os.path.join(out, 'remap.csv'), 'w') as remap_csv:
        rm.remap(r1, r2, prelim, remap_csv, gzip=True, work_path=out,
                 debug_file_prefix=os.path.join(out, 'dbg'))
    sh = session.shard()
    assert sh is not None and sh.world == 2
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

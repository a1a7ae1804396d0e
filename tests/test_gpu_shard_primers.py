"""trim_fastqs.trim() with 5' primers split over the ranks of a job: 2 ranks
on the test box's one GPU (gloo) each censor and trim their block of the fuzz
file's records (censor_fastq._censor_block) and write their gzip members at
their offset of the destination.  The decompressed destination, the two
summaries and the statistics summed over the ranks must equal the single-rank
run."""
import gzip
import io
import json
import os
import socket
import subprocess
import sys
import zlib

import pytest

import primer_cases
import trim_cases
from micall_amd import trim_fastqs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'gpu_primer_worker.py')


def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_sharded_primers_equal_single_rank(tmp_path):
    world = 2
    data = primer_cases.fuzz_fastq()
    lists = primer_cases.fuzz_primers()
    (tmp_path / 'in.fastq.gz').write_bytes(gzip.compress(data, 1))
    job = dict(primers1=lists[0], primers2=lists[1], bad_cycles=trim_cases.fuzz_bad_rows())
    (tmp_path / 'job.json').write_text(json.dumps(job))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_port()), WORLD_SIZE=str(world),
               MICALL_DIST_BACKEND='gloo', MICALL_HIP_DEVICE='0')
    procs = [subprocess.Popen([sys.executable, WORKER, '--dir', str(tmp_path)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(world)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0] * world, codes
    # the single-rank run, in this process
    dest, summary, primer_summary = io.BytesIO(), io.StringIO(), io.StringIO()
    single = trim_fastqs.trim(io.BytesIO(gzip.compress(data, 1)), dest, (), bad_cycles_reader=job['bad_cycles'],
                              summary_file=summary, primers1=lists[0], primers2=lists[1],
                              primer_summary_file=primer_summary)
    want, stats = primer_cases.fuzz_expected(True)[:2]
    assert gzip.decompress(dest.getvalue()) == want and primer_cases.stats_of(single) == stats
    out = (tmp_path / 'out.fastq.gz').read_bytes()
    assert gzip.decompress(out) == want
    # each rank wrote its own block: one gzip member per rank
    members, rest = 0, out
    while rest:
        d = zlib.decompressobj(31)
        d.decompress(rest)
        members, rest = members + 1, d.unused_data
    assert members == world
    for r in range(world):    # every rank returns the sums
        assert json.load(open(tmp_path / ('rank%d.json' % r))) == single
    assert (tmp_path / 'summary.csv').read_text() == summary.getvalue()
    assert (tmp_path / 'primer_summary.csv').read_text() == primer_summary.getvalue()

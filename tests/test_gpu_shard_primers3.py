"""trim_fastqs.trim() with 3' primers split over the ranks of a job: 3 ranks
on the test box's one GPU (gloo) each censor and trim their block of the
chain file's records (bad cycles, adapters, 5' primers, 3' primers as
'mates') and write their gzip members at their offset of the destination.
The decompressed destination, the two summaries and the statistics summed
over the ranks must equal the single-rank run and the oracles."""
import gzip
import io
import json
import os
import socket
import subprocess
import sys
import zlib

import pytest

import primer3_cases
import primer_cases
import trim_cases
from micall_amd import trim_fastqs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'gpu_primer3_worker.py')


def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_sharded_primers3_equal_single_rank(tmp_path):
    world = 3
    data = primer3_cases.chain_fastq()
    five = primer3_cases.CHAIN_PRIMERS
    (tmp_path / 'in.fastq.gz').write_bytes(gzip.compress(data, 1))
    job = dict(adapter=primer3_cases.ADAPTER, min_overlap=trim_cases.MIN_OVERLAP, primers1=five[0],
               primers2=five[1], bad_cycles=trim_cases.fuzz_bad_rows())
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
    dest, summary, primer3_summary = io.BytesIO(), io.StringIO(), io.StringIO()
    single = trim_fastqs.trim(io.BytesIO(gzip.compress(data, 1)), dest, job['adapter'],
                              bad_cycles_reader=job['bad_cycles'], summary_file=summary,
                              min_overlap=job['min_overlap'], primers1=five[0], primers2=five[1],
                              primers3_1='mates', primers3_2='mates', primer3_summary_file=primer3_summary)
    want, adapter_stats, stats5, stats3 = primer3_cases.chain_expected()[:4]
    assert gzip.decompress(dest.getvalue()) == want
    assert trim_cases.stats_of(single) == adapter_stats and primer_cases.stats_of(single) == stats5
    assert primer3_cases.stats_of(single) == stats3
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
    assert (tmp_path / 'primer3_summary.csv').read_text() == primer3_summary.getvalue()

"""
tests/golden/gen_debug_reports.py -- fixture generation, runs in the dev
container only (needs the reference through refharness; nothing imports it at
test time).  The files it writes hold data only.

  reports   tests/golden/debug_reports.json: the reference's
            remap.sam_to_conseqs(debug_reports=...) on the two debug calls of
            micall/tests/remap_test.py and on every seeded text of
            tests/debug_report_cases.py.  Per case: name, sam (a seeded text
            as sam_sha256 only: debug_report_cases.golden_cases generates it
            again), quality_cutoff, keys [[rname, pos]] and reports [string
            per key]; one case per line.
  files     tests/golden/debug_files/<case>/: the reference's
            remap(debug_file_prefix=...) on the committed inputs of
            tests/golden/e2e/<case>/ (the recipe of gen_golden.py's e2e):
            every <n>_debug_ref.fasta / <n>_debug.sam gzip'd, and
            last_conseqs.json.gz, the reference's sam_to_conseqs(seeds=...,
            is_filtered=True, filter_coverage=5) of the last pass's SAM file
            (the consensus a further pass would have mapped to).  A case with
            a file above MAX_BYTES is dropped and named.

usage: python tests/golden/gen_debug_reports.py [reports] [files]
"""
import glob
import gzip
import io
import json
import os
import shutil
import sys
import tempfile

import refharness

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, 'oracle'), os.path.join(REPO, 'micall-lite_amd'), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FILE_CASES = ('micro_2070A-PR', 'micro_2090A-HCV', 'syn_maxremaps', 'syn_unpaired300')
MAX_BYTES = 1 << 20            # no committed file above 1 MiB
REMAP_TEST_CASES = ('testDebugReports', 'testDebugReportsOnReverseRead')


def gen_reports():
    refharness.setup()
    from micall.core import remap
    import debug_report_cases as drc
    records = []
    real = remap.sam_to_conseqs

    def recorder(samfile, quality_cutoff=0, debug_reports=None, *args, **kw):
        text = samfile.getvalue() if hasattr(samfile, 'getvalue') else samfile.read()
        keys = list(debug_reports) if debug_reports else None
        result = real(io.StringIO(text), quality_cutoff, debug_reports, *args, **kw)
        if keys:
            records.append(dict(name='remap_test{}'.format(len(records)), sam=text,
                                quality_cutoff=quality_cutoff, keys=[list(k) for k in keys],
                                reports=[debug_reports[k] for k in keys]))
        return result

    remap.sam_to_conseqs = recorder
    try:
        import micall.tests.remap_test as rt
        suite = rt.SamToConseqsTest
        for name in REMAP_TEST_CASES:
            suite(name).debug()
    finally:
        remap.sam_to_conseqs = real
    assert len(records) == len(REMAP_TEST_CASES)
    reached = drc.covered()
    for name, sam, q, keys in drc.cases():
        reports = {tuple(k): None for k in keys}
        real(io.StringIO(sam), q, reports)
        records.append(dict(name=name, sam_sha256=drc.sha(sam), quality_cutoff=q,
                            keys=[list(k) for k in keys],
                            reports=[reports[tuple(k)] for k in keys]))
    path = os.path.join(HERE, 'debug_reports.json')
    with open(path, 'w') as f:
        head = dict(source='reference remap.sam_to_conseqs(debug_reports=...): remap_test.py '
                           'debug calls, then the texts of tests/debug_report_cases.py',
                    reached=reached)
        f.write(json.dumps(head)[:-1] + ', "cases": [\n')
        f.write(',\n'.join(json.dumps(r) for r in records) + '\n]}\n')
    print('debug_reports: {} cases, {} bytes'.format(len(records), os.path.getsize(path)))


def gen_files():
    refharness.setup()
    import gen_golden
    from micall.core.prelim_map import prelim_map
    from micall.core import remap as ref
    from micall.core import project_config
    shim = os.path.join(REPO, 'oracle', 'shim_bin')
    config = project_config.ProjectConfig.loadDefault().config
    seeds = {name: ''.join(vals['reference']) for name, vals in config['regions'].items()}
    for case in FILE_CASES:
        src = os.path.join(HERE, 'e2e', case)
        r1 = os.path.join(src, 'R1.fastq.gz')
        r2 = os.path.join(src, 'R2.fastq.gz')
        r2 = r2 if os.path.exists(r2) else None
        work = tempfile.mkdtemp(prefix='dbg_')
        cwd = os.getcwd()
        os.chdir(work)
        try:
            prelim = os.path.join(work, 'prelim.csv')
            with open(prelim, 'w') as handle:
                prelim_map(r1, r2, handle, bt2_path=os.path.join(shim, 'bowtie2'),
                           bt2build_path=os.path.join(shim, 'bowtie2-build-s'), nthreads=1,
                           gzip=True, work_path=work)
            with open(prelim) as pre, open(os.path.join(work, 'remap.csv'), 'w') as out:
                ref.remap(r1, r2, pre, out, work_path=work, bt2_path=os.path.join(shim, 'bowtie2'),
                          bt2build_path=os.path.join(shim, 'bowtie2-build-s'), nthreads=1,
                          gzip=True, keep=True, debug_file_prefix=os.path.join(work, 'dbg'))
            made = sorted(glob.glob(os.path.join(work, 'dbg_remap*')))
            sams = [m for m in made if m.endswith('_debug.sam')]
            assert made and len(made) == 2 * len(sams), made
            last = os.path.join(work, 'dbg_remap{}_debug.sam'.format(len(sams)))
            with open(last) as f:
                last_conseqs = ref.sam_to_conseqs(f, ref.CONSENSUS_Q_CUTOFF, seeds=seeds,
                                                  is_filtered=True, filter_coverage=5)
            dst = os.path.join(HERE, 'debug_files', case)
            shutil.rmtree(dst, ignore_errors=True)
            os.makedirs(dst)
            sizes = {}
            for m in made:
                name = os.path.basename(m)[len('dbg_'):] + '.gz'
                with open(m, 'rb') as f:
                    gen_golden._gz_write(os.path.join(dst, name), f.read())
                sizes[name] = os.path.getsize(os.path.join(dst, name))
            gen_golden._gz_write(os.path.join(dst, 'last_conseqs.json.gz'),
                                 json.dumps(dict(passes=len(sams), conseqs=last_conseqs)))
            if max(sizes.values()) > MAX_BYTES:
                shutil.rmtree(dst)
                print('debug_files: {} DROPPED, {}'.format(case, sizes))
            else:
                print('debug_files: {} {} passes {}'.format(case, len(sams), sizes))
        finally:
            os.chdir(cwd)
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    what = sys.argv[1:] or ['reports', 'files']
    if 'reports' in what:
        gen_reports()
    if 'files' in what:
        gen_files()

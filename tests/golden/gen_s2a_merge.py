"""
tests/golden/gen_s2a_merge.py -- fixture generation, runs in the dev
container only (needs the reference through refharness; nothing imports it at
test time).

Writes tests/golden/s2a_merge_paths.json: the reference's
micall.core.sam2aln.sam2aln() with its SAM2ALN_Q_CUTOFFS list patched (as
gen_golden_qcuts.py does), on every directed text of
tests/s2a_merge_cases.py at every one of its q-cutoff lists.

Per case: its name, the path it targets, the SHA-256 and length of the
generated input text (a drifting generator then asks for a regenerated fixture
instead of comparing against stale results) and one entry per list with
aligned.csv, insert.csv and failed.csv -- a text longer than TEXT_LIMIT bytes
as its length and SHA-256 ('sha256', 'bytes'), the convention of
sam2aln_qcuts.json -- and their row counts.  Where the reference raises (the
all-gap unit), the entry holds the exception's class and message instead.
Texts the library itself refuses (a span too long for LDS) have no reference
value and no entry.

The file holds data only.

usage: python tests/golden/gen_s2a_merge.py
"""
import io
import json
import os
import sys

import refharness

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(REPO, 'oracle'), os.path.join(REPO, 'micall-lite_amd'), os.path.join(REPO, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import s2a_merge_cases as mc  # noqa: E402


def main():
    refharness.setup()
    from micall.core import sam2aln as ref

    def run(text, cuts):
        saved = ref.SAM2ALN_Q_CUTOFFS
        ref.SAM2ALN_Q_CUTOFFS = list(cuts)
        try:
            al, ins, fa = io.StringIO(), io.StringIO(), io.StringIO()
            ref.sam2aln(io.StringIO(text), al, ins, fa)
        finally:
            ref.SAM2ALN_Q_CUTOFFS = saved
        return al.getvalue(), ins.getvalue(), fa.getvalue()

    cases = []
    for c in mc.cases():
        entry = dict(name=c.name, path=c.path, input=c.sha(), runs=[])
        for cuts in ([] if c.refused else c.lists):
            try:
                al, ins, fa = run(c.text, cuts)
            except Exception as e:      # stored, and the tests ask the same of the oracle
                entry['runs'].append(dict(q_cutoffs=cuts,
                                          raises={'class': type(e).__name__, 'message': str(e)}))
                continue
            entry['runs'].append(dict(q_cutoffs=cuts, aligned=mc.stored(al), insert=mc.stored(ins),
                                      failed=mc.stored(fa),
                                      rows=[t.count('\n') - 1 for t in (al, ins, fa)]))
        cases.append(entry)
    path = os.path.join(HERE, 's2a_merge_paths.json')
    with open(path, 'w') as f:
        json.dump(dict(source='reference micall.core.sam2aln.sam2aln outputs with SAM2ALN_Q_CUTOFFS '
                              'patched, on the texts of tests/s2a_merge_cases.py', cases=cases),
                  f, indent=0)
    print('s2a_merge_paths: {} cases, {} runs, {} bytes'.format(
        len(cases), sum(len(c['runs']) for c in cases), os.path.getsize(path)))


if __name__ == '__main__':
    main()

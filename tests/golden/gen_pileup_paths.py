"""
tests/golden/gen_pileup_paths.py -- fixture generation, runs in the dev
container only (needs the reference through refharness and the built
library for its constants; nothing imports it at test time).

Writes tests/golden/pileup_paths.json: the reference's
micall.core.remap.sam_to_conseqs() on every SAM text of
tests/pileup_path_cases.py at quality cutoffs 0 and 20, with its
counts_to_conseqs wrapped to capture the refmap it builds.  Per case and
cutoff:

  sam       length and SHA-256 of the generated text (a guard against
            generator drift: the tests regenerate the text and compare)
  conseqs   {reference: consensus}, in the reference's order
  order     the reference order of refmap
  counters  {reference: {position: {token: count}}} without empty positions
            in the canonical JSON form of pileup_path_cases.canonical_counters

conseqs values and counters longer than TEXT_LIMIT bytes are stored as their
length and SHA-256 (the stored() pattern of gen_golden_qcuts.py): equality is
what the tests check.  The file holds data only.

usage: python tests/golden/gen_pileup_paths.py
"""
import io
import json
import os
import sys
import time

import refharness

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, 'oracle'), os.path.join(REPO, 'micall-lite_amd'), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    refharness.setup()
    from micall.core import remap as ref

    import pileup_path_cases as ppc

    captured = {}
    original = ref.counts_to_conseqs

    def capturing(refmap):
        captured['order'] = list(refmap)
        captured['counters'] = ppc.canonical_counters(refmap)   # before the defaultdicts grow
        return original(refmap)

    out = []
    ref.counts_to_conseqs = capturing
    try:
        for case in ppc.cases():
            for q in ppc.Q_CUTOFFS:
                t0 = time.time()
                conseqs = ref.sam_to_conseqs(io.StringIO(case.sam), q)
                out.append(dict(name=case.name, quality_cutoff=q, sam=case.sha(),
                                conseqs={k: ppc.stored(v) for k, v in conseqs.items()},
                                order=captured['order'], counters=ppc.stored(captured['counters'])))
                print('{} q={}: {:.2f} s'.format(case.name, q, time.time() - t0))
    finally:
        ref.counts_to_conseqs = original
    path = os.path.join(HERE, 'pileup_paths.json')
    with open(path, 'w') as f:
        json.dump(dict(source='reference micall.core.remap.sam_to_conseqs: conseqs and the refmap '
                              'handed to counts_to_conseqs, on the texts of tests/pileup_path_cases.py',
                       cases=out), f, indent=0)
    print('pileup_paths: {} cases, {} bytes'.format(len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()

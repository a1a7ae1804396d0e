"""
tests/golden/gen_golden_qcuts.py -- fixture generation, runs in the dev
container only (needs the reference through refharness; nothing imports it at
test time).

Writes tests/golden/sam2aln_qcuts.json: the reference's
micall.core.sam2aln.sam2aln() with its SAM2ALN_Q_CUTOFFS list patched, on

  * the eight-base example whose cutoff groups come out in first-success
    order (10, 0, 15 for the list [15, 10, 0]),
  * every remap_csv of tests/golden/sam2aln_e2e.json,
  * the two smallest tests/golden/e2e/*/remap.csv.gz,
  * one unpaired text (flags 0 / 16),

each with the lists [0, 10, 15], [15, 10, 0], [15, 15], [20] and [0, 93].

The file holds data only.  To stay under 300 kB with every text at every
list, a text that sam2aln_e2e.json already holds is named by its index there
('e2e_json_case') instead of being copied, and an output longer than
TEXT_LIMIT bytes is stored as its length and SHA-256 ('sha256', 'bytes')
instead of its text: byte equality is what the tests check, and a digest
checks exactly that.

usage: python tests/golden/gen_golden_qcuts.py
"""
import gzip
import hashlib
import io
import json
import os

import refharness

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD = 'qname,flag,rname,pos,mapq,cigar,rnext,pnext,tlen,seq,qual\n'
LISTS = [[0, 10, 15], [15, 10, 0], [15, 15], [20], [0, 93]]
TEXT_LIMIT = 2048


def tiny_text():
    rows = []
    for name, qual in (('p1', '-----???'), ('p2', '????????'), ('p3', '!!!!!!!!')):
        for flag in (99, 147):
            rows.append('{},{},R,1,44,8M,=,1,8,ACGTACGT,{}\n'.format(name, flag, qual))
    return HEAD + ''.join(rows)


def unpaired_text():
    """Single reads (flag bit 1 clear): mseq = seq1 at every cutoff, whatever
    the qualities; Ns in the read decide manyNs; one read twice (count 2), a
    deletion, an insertion, a second reference."""
    rows = [
        'u1,0,R,3,44,8M,*,0,0,ACGTACGT,!!!!!!!!\n',
        'u2,16,R,3,44,8M,*,0,0,ACGTACGT,IIIIIIII\n',
        'u3,0,R,1,44,3M2D3M,*,0,0,ACGTAC,#-#-#-\n',
        'u4,16,R,2,44,2M2I4M,*,0,0,ACGGTACG,IIII--##\n',
        'u5,0,R,1,44,8M,*,0,0,ANNNNNCG,IIIIIIII\n',
        'u6,0,S,5,44,6M,*,0,0,TTGACC,555555\n',
    ]
    return HEAD + ''.join(rows)


def stored(text):
    if len(text) <= TEXT_LIMIT:
        return text
    data = text.encode()
    return dict(sha256=hashlib.sha256(data).hexdigest(), bytes=len(data))


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

    texts = [dict(name='tiny', remap_csv=tiny_text())]
    with open(os.path.join(HERE, 'sam2aln_e2e.json')) as f:
        e2e_json = json.load(f)['cases']
    for k, case in enumerate(e2e_json):
        texts.append(dict(name='e2e_json[{}] {}'.format(k, case['source']), e2e_json_case=k))
    e2e = os.path.join(HERE, 'e2e')
    by_size = sorted(os.listdir(e2e),
                     key=lambda c: (os.path.getsize(os.path.join(e2e, c, 'remap.csv.gz')), c))
    for case in by_size[:2]:
        with gzip.open(os.path.join(e2e, case, 'remap.csv.gz'), 'rt') as f:
            texts.append(dict(name='e2e/' + case, remap_csv=f.read()))
    texts.append(dict(name='unpaired', remap_csv=unpaired_text()))

    cases = []
    for t in texts:
        text = t['remap_csv'] if 'remap_csv' in t else e2e_json[t['e2e_json_case']]['remap_csv']
        for cuts in LISTS:
            al, ins, fa = run(text, cuts)
            case = dict(t)
            case.update(q_cutoffs=cuts, aligned=stored(al), insert=stored(ins), failed=stored(fa))
            cases.append(case)
    path = os.path.join(HERE, 'sam2aln_qcuts.json')
    with open(path, 'w') as f:
        json.dump(dict(source='reference micall.core.sam2aln.sam2aln outputs with '
                              'SAM2ALN_Q_CUTOFFS patched', cases=cases), f, indent=0)
    print('qcuts: {} cases, {} bytes'.format(len(cases), os.path.getsize(path)))


if __name__ == '__main__':
    main()

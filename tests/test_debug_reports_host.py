"""CPU checks of the sam_to_conseqs drop-in's host parts (no GPU):

  * mh_sam_parse (csrc/mh_sam.cpp: remap.matchmaker with include_singles,
    remap.py:853-889) against pileup_path_cases.rows_of on every SAM text of
    pileup_golden.json and debug_reports.json, and on edge texts;
  * the Python restatement of the watched count
    (debug_report_cases.watched), formatted by the product's
    consensus.format_debug_report, against the reference's strings of
    debug_reports.json: this pins both, and the GPU tests then hold the
    kernel's histogram equal to the restatement's;
  * the parser compiled alone with AddressSanitizer and UBSan, run over the
    same edge texts and over one golden text cut at every byte.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import debug_report_cases as drc
import pileup_path_cases
from micall_amd import _native
from micall_amd.consensus import format_debug_report

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'micall-lite_amd', 'csrc')
ROW = 'q1\t99\tr1\t5\t44\t4M\t=\t5\t4\tACGT\tFFFF\n'
SQ = '@SQ\tSN:r1\tLN:100\n'


@pytest.fixture(scope='module')
def report_cases(golden_dir):
    return drc.golden_cases(os.path.join(golden_dir, 'debug_reports.json'))


def _golden_sams(golden_dir):
    with open(os.path.join(golden_dir, 'pileup_golden.json')) as f:
        out = [c['sam'] for c in json.load(f)['cases']]
    return out + [c['sam'] for c in drc.golden_cases(os.path.join(golden_dir, 'debug_reports.json'))]


def _same_rows(sam):
    want_names, _pairs, want = pileup_path_cases.rows_of(sam)
    names, ends, got = _native.sam_parse(sam)
    assert names == want_names
    flag, ref, pos, cig_off, n_cig, cig, seq, qual, offs, lens, units = want
    assert got[0].tolist() == flag and got[1].tolist() == ref and got[2].tolist() == pos
    assert got[3].tolist() == cig_off and got[4].tolist() == n_cig
    assert got[5].tolist() == (cig if n_cig and sum(n_cig) else [])
    assert got[6].tobytes() == seq.tobytes() and got[7].tobytes() == qual.tobytes()
    assert got[8].tolist() == [int(x) for x in offs] and got[9].tolist() == lens
    assert got[10].tolist() == units
    # per reference the largest end (POS - 1 + M + D) of a mapped row
    want_ends = [0] * len(names)
    for f, r, p, o, n in zip(flag, ref, pos, cig_off, n_cig):
        if not f & 4:
            span = sum(w >> 4 for w in cig[o:o + n] if w & 15 in (0, 2))
            want_ends[r] = max(want_ends[r], p - 1 + span)
    assert ends.tolist() == want_ends
    return names, got


def test_sam_parse_equals_rows_of_on_every_golden_text(golden_dir):
    sams = _golden_sams(golden_dir)
    assert len(sams) > 60
    for sam in sams:
        _same_rows(sam)


def test_sam_parse_edge_texts():
    names, ends, args = _native.sam_parse('')
    assert names == [] and len(args[0]) == 0 and len(args[10]) == 0
    names, ends, args = _native.sam_parse('@HD\tVN:1.0\n' + SQ + '@PG\tID:x\n')
    assert names == ['r1'] and ends.tolist() == [0] and len(args[0]) == 0
    # no final newline: the last line counts; '\n' alone is stripped
    for text in (SQ + ROW[:-1], SQ + ROW):
        names, got = _same_rows(text)
        assert got[10].tolist() == [0, -1] and got[6].tobytes() == b'ACGT'
    # '\r\n' lines: the '\r' stays on the last field.  After LN it does no
    # harm, and on QUAL it is cut off with QUAL at SEQ's length; after SN the
    # header's name is 'r1\r', so a plain r1 row is dropped
    names, got = _same_rows((SQ + ROW).replace('\n', '\r\n'))
    assert names == ['r1'] and got[7].tobytes() == b'FFFF' and got[10].tolist() == [0, -1]
    names, _ends, args = _native.sam_parse('@SQ\tSN:r1\r\n' + ROW.replace('\n', '\r\n'))
    assert names == ['r1\r'] and len(args[0]) == 0
    # two SN values on one @SQ line, the second reference listed once more later
    two = '@SQ\tSN:a\tLN:5\tSN:b\n@SQ\tSN:b\n' + ROW.replace('r1', 'b') + ROW.replace('r1', 'c')
    names, got = _same_rows(two)
    assert names == ['a', 'b'] and got[1].tolist() == [1]
    # three rows of one QNAME: the first two pair, the third is a single
    three = SQ + ROW + ROW.replace('99', '147') + ROW.replace('99', '0')
    names, got = _same_rows(three)
    assert got[10].tolist() == [0, 1, 2, -1] and got[0].tolist() == [99, 147, 0]
    # singles follow the pairs, in the order they were last cached
    mixed = SQ + ROW.replace('q1', 'a') + ROW.replace('q1', 'b') + ROW.replace('q1', 'a')
    names, got = _same_rows(mixed)
    assert got[10].tolist() == [0, 1, 2, -1]
    # a row on a name outside @SQ is dropped, even a short one; a kept row
    # with fewer than eleven fields, or a FLAG / POS that is no integer,
    # raises in the reference (merge_reads) and is refused here by line
    names, _ends, args = _native.sam_parse(SQ + 'q\t0\tother\t1\n' + ROW)
    assert args[10].tolist() == [0, -1]
    for bad, what in ((SQ + ROW + 'q2\t0\tr1\t1\t44\t4M\t=\t1\t0\tACGT\n', 'line 3'),
                      (SQ + 'q2\t0\n', 'line 2'),
                      (SQ + ROW.replace('\t5\t44', '\tx5\t44'), 'POS'),
                      (SQ + ROW.replace('\t99\t', '\t9 9\t'), 'FLAG'),
                      ('@SQ\tSN\n', "':'")):
        with pytest.raises(_native.NativeError) as err:
            _native.sam_parse(bad)
        assert what in str(err.value)
    # an unusable CIGAR is one op 3 (refused when the rows are loaded)
    names, _ends, args = _native.sam_parse(SQ + ROW.replace('4M', '4Q'))
    assert args[5].tolist() == [3] and args[4].tolist() == [1]


def test_texts_reach_every_situation(report_cases):
    reached = drc.covered()
    assert set(reached) == set(drc.FACTS) and all(reached.values())
    # the fixture was generated from these very texts (golden_cases
    # compares each one's SHA-256, cutoff and keys)
    assert [c['name'] for c in report_cases[2:]] == [name for name, _s, _q, _k in drc.cases()]
    for _name, sam, _q, _keys in drc.cases():
        assert sam.count('\n') <= 3 + 1 + 2 * 60


def test_restatement_formatted_equals_the_reference_strings(report_cases):
    assert len(report_cases) == 2 + drc.N_TEXTS
    n_reports = 0
    for c in report_cases:
        keys = [tuple(k) for k in c['keys']]
        counts, first = drc.watched(c['sam'], c['quality_cutoff'], keys)
        got = [format_debug_report(counts[k], first[k]) for k in range(len(keys))]
        assert got == c['reports'], c['name']
        n_reports += sum(1 for r in c['reports'] if r)
    assert n_reports > 300
    # the order of the bases inside a report is the order they were first
    # counted in, not a sorted one
    counts = np.zeros((4, drc.QBINS), dtype=np.uint32)
    first = np.full((4, drc.QBINS), drc.NEVER, dtype=np.int64)
    counts[3, ord('F') - 32], first[3, ord('F') - 32] = 2, 0
    counts[0, ord('I') - 32], first[0, ord('I') - 32] = 1, 1
    counts[3, ord(' ') - 32], first[3, ord(' ') - 32] = 1, 2
    assert format_debug_report(counts, first) == ' {T: 3, A: 1}, F{T: 2, A: 1}, I{A: 1}'
    assert format_debug_report(np.zeros_like(counts), first) == ''


SANITIZED_MAIN = r'''
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "micall_hip.h"
namespace mh { void set_error(const char *, ...) {} }
static long run(const char *p, long n)
{
    mh_sam_sizes z;
    if (mh_sam_parse(p, n, &z, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)) return -1;
    std::vector<int32_t> i32[6];
    for (auto &v : i32) v.resize(z.n_rows + 1);
    std::vector<uint32_t> cig(z.n_cigar + 1);
    std::vector<int64_t> off(z.n_rows + 1), units(2 * z.n_units + 1);
    std::vector<uint8_t> seq(z.n_bases + 1), qual(z.n_bases + 1);
    std::vector<char> names(z.names_bytes + 1);
    std::vector<int32_t> ends(z.n_refs + 1);
    if (mh_sam_parse(p, n, &z, i32[0].data(), i32[1].data(), i32[2].data(), i32[3].data(),
                     i32[4].data(), cig.data(), off.data(), i32[5].data(), seq.data(), qual.data(),
                     units.data(), names.data(), ends.data())) return -1;
    return (long)z.n_rows;
}
int main(int argc, char **argv)
{
    long ok = 0, refused = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const bool every_cut = a == 1;   // the first file is cut at every byte
        for (size_t n = every_cut ? 0 : text.size(); n <= text.size(); ++n) {
            // an exact-size copy: a read past the end is a heap overflow
            std::vector<char> copy(text.begin(), text.begin() + n);
            (run(copy.data(), (long)n) < 0 ? refused : ok) += 1;
        }
    }
    std::printf("%ld parsed, %ld refused\n", ok, refused);
    return 0;
}
'''


def test_parser_alone_under_asan_and_ubsan(tmp_path, report_cases):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    cxx = hipcc if os.path.exists(hipcc) else shutil.which('clang++') or shutil.which('g++')
    assert cxx, 'no C++ compiler'
    main_cpp = tmp_path / 'sam_main.cpp'
    main_cpp.write_text(SANITIZED_MAIN)
    exe = str(tmp_path / 'sam_san')
    lang = ['-x', 'c++'] if cxx == hipcc else []
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I' + os.path.join(REPO, 'include'), '-I' + CSRC]
                   + lang + [str(main_cpp), os.path.join(CSRC, 'mh_sam.cpp'), '-o', exe], check=True)
    texts = [report_cases[0]['sam'] + report_cases[2]['sam'][:6000], '', SQ, SQ + ROW[:-1],
             (SQ + ROW).replace('\n', '\r\n'), SQ + 'q2\t0\n', SQ + ROW.replace('\t5\t44', '\tx\t44'),
             '@SQ\tSN:a\tSN:b\n' + ROW.replace('r1', 'b'), SQ + ROW * 3, '\n\n', '@SQ\tSN\n',
             SQ + ROW.replace('4M', '99999999999999999999M'), SQ + ROW.replace('\t5\t', '\t99999999999\t')]
    paths = []
    for k, text in enumerate(texts):
        path = tmp_path / 'text{}.sam'.format(k)
        path.write_bytes(text.encode())
        paths.append(str(path))
    run = subprocess.run([exe] + paths, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1'))
    assert run.returncode == 0, run.stderr[-3000:]
    assert 'parsed' in run.stdout and 'runtime error' not in run.stderr

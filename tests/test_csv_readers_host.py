"""The one CSV reader (csrc/mh_csv.h) and the prelim.csv parse built on it
(csrc/mh_prelim.cpp, mh_prelim_parse), on the host: against a restatement on
Python's own csv module (prelim_cases.restate) for every block count, against
what the previous reader returned for the golden prelim.csv files
(tests/golden/prelim_rows_info.json, recorded from Context.rows_load_csv
before the readers were unified), and as a stand-alone program under the
sanitizers (tests/csv_readers_main.cpp)."""
import base64
import glob
import gzip
import json
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import prelim_cases as pc
from micall_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'micall-lite_amd', 'csrc')
THREADS = (1, 2, 3, 8)


def _quoted_newlines(body):
    """Offsets of the '\\n' inside a quoted field of a CSV body."""
    inside, out = False, set()
    for i, ch in enumerate(body):
        if ch == '"':
            inside = not inside
        elif ch == '\n' and inside:
            out.add(i)
    return out


def test_the_inner_newline_text_puts_even_splits_inside_the_quotes():
    body = pc.INNER_NEWLINE[len(pc.HEAD) + 1:]
    quoted = _quoted_newlines(body)
    for t in (2, 3):
        for k in range(1, t):
            assert body.index('\n', len(body) * k // t) in quoted


@pytest.mark.parametrize('name', sorted(pc.TEXTS))
def test_prelim_parse_equals_the_restatement_for_every_block_count(name):
    text = pc.TEXTS[name]
    want = pc.restate(text)
    for t in THREADS:
        pc.assert_same(_native.prelim_parse(text, pc.REFNAMES, threads=t), want, (name, t))


def test_what_the_edge_texts_hold():
    # the texts do reach the situations they are named for
    r = {name: pc.restate(text) for name, text in pc.TEXTS.items()}
    assert r['permuted'] == r['plain'] == r['crlf'] == r['no_final_newline']
    assert r['plain'][0][10] == [0, 1, 2, 3, 4, -1] and r['plain'][0][7] == b'IIIIIIIIIIHHHHHHHHJJGGGGG'
    assert r['quoted_qual'][0][7] == b'II,I"' + b'"JJJJ' + b'HHHHH'
    assert r['quoted_qname'][0][10] == [0, 1, 2, 3]
    assert r['inner_newline'][1]['n_rows'] == 4 and r['inner_newline'][0][10] == [0, 2, 1, -1, 3, -1]
    assert r['after_closing_quote'][0][10] == [0, 1] and r['after_closing_quote'][0][7] == b'IIIII' * 2
    assert r['lone_cr'][1]['n_rows'] == 3 and r['blank_lines'][1]['n_rows'] == 2
    assert r['unknown_rnames'][1]['unknown'] == ['other', '*']
    assert [i[0] for i in r['unknown_rnames'][1]['info']] == [0, -1, -2, 0, -1, -2, 1]
    assert r['unknown_rnames'][0][10] == [0, 3, 6, -1] and r['unknown_rnames'][1]['present'] == [0, 1]
    assert r['unpaired_mate'][0][10] == [1, 2, 0, -1]
    assert r['three_of_one_qname'][0][10] == [0, 1, 2, -1]
    assert r['cigars'][0][4] == [1, pc.MAXOPS, 1, 1, 2, 0] and r['cigars'][0][5][0] == 3
    assert r['cigars'][0][5][-2:] == [(2 << 4) | 3, 3 << 4]
    assert r['header_only'][1]['n_rows'] == 0


@pytest.mark.parametrize('name', sorted(pc.ERRORS))
def test_prelim_parse_errors(name):
    text, message = pc.ERRORS[name]
    for t in THREADS:
        with pytest.raises(_native.NativeError) as err:
            _native.prelim_parse(text, pc.REFNAMES, threads=t)
        assert message in str(err.value)


def _golden_prelims(golden_dir):
    paths = sorted(glob.glob(os.path.join(golden_dir, 'e2e', '*', 'prelim.csv.gz')) +
                   glob.glob(os.path.join(golden_dir, 'chain', '*', 'prelim.csv.gz')))
    return {'/'.join(p.split(os.sep)[-3:-1]): p for p in paths}


def test_golden_prelim_files_equal_the_restatement_and_the_previous_reader(golden_dir):
    with open(os.path.join(golden_dir, 'prelim_rows_info.json')) as f:
        recorded = json.load(f)
    refnames = recorded['refnames']
    files = _golden_prelims(golden_dir)
    assert sorted(files) == sorted(recorded['files']) and len(files) >= 22
    for key, path in files.items():
        with gzip.open(path, 'rt', newline='') as f:
            text = f.read()
        rec = recorded['files'][key]
        want = pc.restate(text, refnames)
        for t in THREADS:
            got = _native.prelim_parse(text, refnames, threads=t)
            pc.assert_same(got, want, (key, t))
            info = np.frombuffer(zlib.decompress(base64.b64decode(rec['info_zlib_b64'])),
                                 dtype='<i4').reshape(-1, 4)
            assert got[1]['n_rows'] == rec['n_rows'] and got[1]['n_units'] == rec['n_units'], key
            assert np.array_equal(got[1]['info'], info), key
            assert got[1]['present'].tolist() == rec['present'] and got[1]['unknown'] == rec['unknown'], key


PY_INT_TEXTS = ['12', ' 12 ', '+12', '-12', '\t12\f', '', '+', '1 2', '1_2', '12a', '99999999999']


def _int_or_none(text):
    try:
        return int(text)
    except ValueError:
        return None


SAM = '@SQ\tSN:r1\tLN:100\nq1\t{}\tr1\t5\t44\t4M\t=\t5\t4\tACGT\tFFFF\n'


def test_py_int_through_the_sam_flag_is_pythons_int_within_int32():
    # FLAG is a tab-split field: every text without a tab reaches py_int as it is
    for text in PY_INT_TEXTS:
        if '\t' in text:
            continue
        want = _int_or_none(text)
        if text == '1_2':
            want = None     # the known, unchanged gap: int() takes '1_2', py_int refuses it
        if want is not None and not -2 ** 31 <= want < 2 ** 31:
            want = None     # the callers' int32 range check: '99999999999'
        try:
            got = int(_native.sam_parse(SAM.format(text))[2][0][0])
        except _native.NativeError as err:
            assert 'FLAG is not an integer' in str(err)
            got = None
        assert got == want, repr(text)


pytest_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """tests/csv_readers_main.cpp built under ASan + UBSan and under TSan."""
    out = tmp_path_factory.mktemp('csv_readers')
    builds = {}
    for san in ('address,undefined', 'thread'):
        exe = str(out / ('csv_readers_' + san.split(',')[0]))
        cmd = ['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=' + san,
               '-fno-sanitize-recover=all', '-I', CSRC, '-I', os.path.join(REPO, 'include'),
               os.path.join(REPO, 'tests', 'csv_readers_main.cpp')] + \
              [os.path.join(CSRC, n) for n in ('mh_prelim.cpp', 'mh_sam.cpp', 'mh_gunzip.cpp',
                                               'mh_pinflate.cpp')] + \
              ['-o', exe, '-lz', '-lpthread', '-ldl']
        builds[exe] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for exe, proc in builds.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0, log[-4000:]
    return list(builds)


@pytest_gxx
def test_py_int_alone_is_pythons_int(programs):
    run = subprocess.run([programs[0], 'pyint'] + PY_INT_TEXTS, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    got = [None if line == 'no' else int(line.split()[1]) for line in run.stdout.splitlines()]
    want = [_int_or_none(t) for t in PY_INT_TEXTS]
    assert want[PY_INT_TEXTS.index('1_2')] == 12
    want[PY_INT_TEXTS.index('1_2')] = None      # the known, unchanged gap
    assert got == want


@pytest_gxx
def test_cuts_and_prelim_parse_under_the_sanitizers(programs, tmp_path, golden_dir):
    paths = []
    for name, text in list(pc.TEXTS.items()) + [(k, v[0]) for k, v in pc.ERRORS.items()]:
        paths.append(str(tmp_path / (name + '.csv')))
        with open(paths[-1], 'w', newline='') as f:
            f.write(text)
    golden = str(tmp_path / 'golden_prelim.csv')
    with gzip.open(_golden_prelims(golden_dir)['e2e/micro_2100A-HCV-1337B-V3LOOP'], 'rb') as f, \
            open(golden, 'wb') as g:
        g.write(f.read())
    assert os.path.getsize(golden) > 2048
    # every byte offset of the first 2 KB, in four ranges per build side by side
    cmds = [[exe, 'texts'] + paths for exe in programs] + \
           [[exe, 'truncate', golden, str(lo), str(lo + 512 + (lo == 1536))]
            for exe in programs for lo in range(0, 2048, 512)]
    runs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for cmd in cmds]
    for proc in runs:
        log = proc.communicate(timeout=300)[0]
        assert proc.returncode == 0, log[-4000:]
        assert 'csv_readers ok' in log

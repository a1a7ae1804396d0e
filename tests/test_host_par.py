"""The host helpers every translation unit shares (mh_gunzip.h: par_for,
write_all_at, read_all_at) under sanitizers: tests/host_par_main.cpp is built
with csrc/mh_gunzip.cpp and csrc/mh_pinflate.cpp as a stand-alone program,
once with AddressSanitizer + UBSan and once with ThreadSanitizer, and run
directly.  The program's own checks decide its exit status."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'micall-lite_amd', 'csrc')

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


@pytest.fixture(scope='module', params=['address,undefined', 'thread'])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('host_par') / 'host_par')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
           '-fsanitize=' + request.param, '-fno-sanitize-recover=all',
           '-I', CSRC, '-I', os.path.join(REPO, 'include'),
           os.path.join(REPO, 'tests', 'host_par_main.cpp'),
           os.path.join(CSRC, 'mh_gunzip.cpp'), os.path.join(CSRC, 'mh_pinflate.cpp'),
           '-o', exe, '-lz', '-lpthread', '-ldl']
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe


def test_host_helpers_under_sanitizer(program):
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert 'host_par ok' in run.stdout

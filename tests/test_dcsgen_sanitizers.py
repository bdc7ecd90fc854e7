"""CPU-only sanitizer job for the HIP-free part of the DCS generator bank (hackrfdiags_amd/csrc/hrfd_dcsgen.h: the checks, the
grids, the queue rules and the slow loop over one channel), compiled into tests/cpp/san_dcsgen.cc under
-fsanitize=address,undefined and run as a program of its own, the way tests/test_tonegen_sanitizers.py runs san_tonegen.cc."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_dcsgen_helpers_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "san_dcsgen")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(HERE, "cpp", "san_dcsgen.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.join(HERE, "cpp"))
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no runtime for -fsanitize=address,undefined")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "san_dcsgen ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])

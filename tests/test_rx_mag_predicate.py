"""rx_magnitude_unobservable (hackrfdiags_amd/csrc/hrfd_rx_plan.h) -- when a WBFM batch may leave the squelch magnitude
out -- compiled into tests/cpp/san_rx_mag.cc under -fsanitize=address,undefined and swept against the detector by brute
force: gains {0, 1, 40, 2^31 - 43, 2^31, 2^32 - 1} x thresholds {INT32_MIN, -200, -43 - g, -42 - g, -41 - g, 0, INT32_MAX},
every block mean 0 .. 127, the kernels' own 32-bit arithmetic (its wrap at huge gains included).  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_magnitude_predicate_against_the_detector(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "san_rx_mag")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(HERE, "cpp", "san_rx_mag.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.join(HERE, "cpp"))
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no runtime for -fsanitize=address,undefined")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "san_rx_mag ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])

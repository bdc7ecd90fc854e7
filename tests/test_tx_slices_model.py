"""The modulator launch's refusal, time slices and grids (hackrfdiags_amd/csrc/hrfd_tx_slices.h) on the CPU: the header
compiled into tests/cpp/san_tx_slices.cc under -fsanitize=address,undefined and compared with tests/tx_slices_model.py;
the properties of the cuts that need no model; tx_check_call at its bound and one above it; and the refusals of
hrfd_mod_* and hrfd_nco_* that are decided before a device is needed, through the raw C ABI.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from hackrfdiags_amd import _lib
from tests import tx_slices_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = (M.SSB, M.INTERP, M.AM, M.FM, M.WBFM, M.SIG_AM, M.SIG_FM)
CHANNELS = (1, 7, 8, 9, 16, 17, 4096, 4097, 8192, 8193, 65536)
# both sides of: the cascade's tile (128), a unit (64), the recurrence's chunks (step counts that are no multiple of 64 or
# 4), the shortest sliced WBFM call (26 units) and its long tail (72), the shortest sliced FM call (64 units), 2^28 cells
# per row (k_phase_rows' 32-bit offset: n = 2^23 for WBFM)
LENGTHS = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 1536, 1537, 1600, 1601, 1664, 1665, 3968, 4032, 4033,
           4096, 4544, 4545, 4608, 4609, 8192, 8269, 32640, 32641, 65536, 70000, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1)
EINVAL, ENODEV = -1, -2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("tx_slices") / "san_tx_slices")
    base = ["g++", "-x", "c++", "-std=c++17", "-g", "-O1", "-o", out, os.path.join(HERE, "cpp", "san_tx_slices.cc")]
    b = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        b = subprocess.run(base, capture_output=True, text=True)   # no sanitizer runtime here: the comparison still runs
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def run(exe, what, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, what], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout.splitlines()


def test_cuts_against_the_model_and_their_own_terms(exe):
    """every call length up to 70000 samples and a band below each refusal bound: the header's cuts are the model's, and
    without a model: they increase strictly, end with the call, fall on multiples of 128 samples before that, are at most
    kMaxSlices (the harness has guard words behind the event pairs' count), and a call is in one piece exactly when it
    has at most 24 units counted even (WBFM) or fewer than 64 (FM)"""
    top = M.max_n(M.SSB, 1)
    assert M.WBFM_MAX_N == 67108735 and top == 128 * (2 ** 21 - 1)
    lengths = list(range(1, 70001)) + list(range(M.WBFM_MAX_N - 300, M.WBFM_MAX_N + 1)) + list(range(top - 300, top + 1))
    out = run(exe, "cuts", "".join("%d\n" % n for n in lengths))
    assert len(out) == len(lengths)
    for n, line in zip(lengths, out):
        t = line.split()
        fm = t.index("fm")
        assert int(t[0]) == n and t[1] == "wbfm"
        wb = [int(x) for x in t[4:fm]]
        nt = (n + 63) // 64
        assert int(t[2]) == (len(wb) > 1) == ((nt & ~1) > 24), line
        assert int(t[3]) == len(wb) <= M.MAX_SLICES and wb == M.wbfm_cuts(n), (line, M.wbfm_cuts(n))
        f = [int(x) for x in t[fm + 2:]]
        assert int(t[fm + 1]) == (len(f) == 4) == (nt >= 64), line
        assert f == (M.fm_cuts(n) if nt >= 64 else []), (line, M.fm_cuts(n))
        for cuts in (wb, f[1:]):
            assert all(a < b for a, b in zip([0] + cuts, cuts)), line
            assert not cuts or (cuts[-1] == n and all(c % 128 == 0 for c in cuts[:-1])), line


def grid_cases():
    for kind in KINDS:
        for ch in CHANNELS:
            top = M.max_n(kind, ch)
            for n in sorted(set(LENGTHS + (top - 129, top - 128, top - 1, top, top + 1, top + 128, 2 ** 32 - 1))):
                for scan_kind in ((0, 1, 2) if kind in (M.FM, M.WBFM) and n <= 70000 else (0,)):
                    yield kind, ch, n, scan_kind
        for ch in (2 ** 24 - 8, 2 ** 24 - 7, 2 ** 24, 2 ** 32 - 1):   # the last bank that has a call at all, and beyond
            for n in (1, 128, 129):
                yield kind, ch, n, 0


def test_grids_against_the_model_and_the_refusal_at_its_bound(exe):
    """every kind, bank size and length of the lists, and each bank's longest accepted call with its neighbours: a call
    is refused exactly when the model refuses it -- accepted at the bound, refused one sample above, with the numbers in
    the text -- and every grid of an accepted call, whole and slice by slice, is the model's (Python's integers: no
    wrap)"""
    todo = list(grid_cases())
    out = run(exe, "grids", "".join("%d %d %d %d\n" % c for c in todo))
    assert len(out) == len(todo) > 3000
    seen = {True: 0, False: 0}
    for (kind, ch, n, scan_kind), line in zip(todo, out):
        ok = M.accepted(kind, ch, n)
        seen[ok] += 1
        if not ok:
            assert line.startswith("%d who: " % EINVAL) and str(ch) in line and str(n) in line, (kind, ch, n, line)
            continue
        assert line.split() == M.grids(kind, ch, n, scan_kind), (kind, ch, n, scan_kind, line)
        assert all(int(x) * 256 < 2 ** 32 for x in line.split() if x.isdigit())
    assert min(seen.values()) > 300
    for kind in KINDS:
        for ch in CHANNELS:
            top = M.max_n(kind, ch)
            assert M.accepted(kind, ch, top) and not M.accepted(kind, ch, top + 1)
    # what hrfd_duc_transmit accepts (n <= 65536, C <= 32768, C n / 4 + C workgroups of its own within the same bound)
    assert all(M.accepted(k, c, min(65536, 4 * (M.MAX_WGS - c) // c)) for k in KINDS for c in (1, 1024, 4096, 32768))


def test_refusals_before_any_device():
    """hrfd_mod_* and hrfd_nco_*: NULL arguments, n_per_channel == 0, a bad kind, no channels and an Nco step that is not
    finite keep HRFD_EINVAL, decided before a device is touched; create without a device is HRFD_ENODEV and leaves no
    handle"""
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.int64)
    p, u32 = C.c_void_p(buf.ctypes.data), C.c_uint32(0)
    for name, args in [("hrfd_mod_reset", (None, 0)), ("hrfd_mod_set_sideband", (None, 0, 1)),
                       ("hrfd_mod_set_modulation_index", (None, 0, 0.5)), ("hrfd_mod_set_deviation", (None, 0, 1000.0)),
                       ("hrfd_mod_process", (None, p, 1, p, C.byref(u32))), ("hrfd_mod_process", (None, p, 0, p, None)),
                       ("hrfd_mod_process_device", (None, p, 1, p, None)), ("hrfd_mod_process_device", (None, p, 0, p, None)),
                       ("hrfd_mod_sync", (None,)), ("hrfd_nco_set_frequency", (None, 0, 1.0)), ("hrfd_nco_reset", (None, 0)),
                       ("hrfd_nco_run", (None, 0, 1, p, p)), ("hrfd_nco_run", (None, 0, 0, p, p))]:
        assert getattr(lib, name)(*args) == EINVAL, name
        assert lib.hrfd_last_error(), name
    for args in ((0, 1, 0), (10, 1, 0), (-1, 1, 0), (M.SSB, 0, 0)):
        h = C.c_void_p(0x1234)
        assert lib.hrfd_mod_create(*args, C.byref(h)) == EINVAL, args
        assert lib.hrfd_last_error().decode().startswith("hrfd_mod_create"), args
    assert lib.hrfd_mod_create(M.SSB, 1, 0, None) == EINVAL
    h = C.c_void_p(0x1234)
    for args in ((0, 8000.0, 1.0, 0), (1, 0.0, 1.0, 0), (1, 1.0, 3.0e6, 0), (1, 8000.0, float("nan"), 0)):
        assert lib.hrfd_nco_create(*args, C.byref(h)) == EINVAL, args
    assert lib.hrfd_nco_create(1, 8000.0, 1.0, 0, None) == EINVAL
    assert lib.hrfd_mod_destroy(None) == 0 and lib.hrfd_nco_destroy(None) == 0
    if lib.hrfd_device_count() == 0:
        for name, args in (("hrfd_mod_create", (M.WBFM, 4, -1)), ("hrfd_nco_create", (4, 8000.0, 100.0, -1))):
            h = C.c_void_p(0x1234)
            assert getattr(lib, name)(*args, C.byref(h)) == ENODEV, name
            assert h.value is None and lib.hrfd_last_error().decode().startswith(name + ": no HIP device visible"), name

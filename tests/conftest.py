import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the suite forces the library's failure and fallback paths through the behaviour-changing hooks of include/hrfd_debug.h;
# they are inert in a process that did not ask for them (read once by libhrfd, so set before it is loaded)
# HRFD_HOOKS_OFF=1 (round 6): the SHIPPED state of the library -- the opt-in is withheld, every behaviour-changing hook answers
# HRFD_ESTATE, the tests that need one skip and the rest (goldens, full-size banks, random walks, short blocks, the closed
# loop over count.raw ...) run on the dispatch a user gets.  tests/test_gpu_hooks_off.py runs the GPU suite that way in a
# fresh child process (the library reads the variable once per process) and reports it group by group.
if os.environ.get("HRFD_HOOKS_OFF") == "1":
    os.environ.pop("HRFD_DEBUG_HOOKS", None)
else:
    os.environ.setdefault("HRFD_DEBUG_HOOKS", "1")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from tests.reflib import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def ref():
    """The reference's own sources compiled by oracle/Makefile (oracle/_ref).
    Built in the dev container (where /root/reference exists) and shipped
    prebuilt to the GPU box.  Where it is absent, the reference's recorded
    answers to these same tests stand in (tests/refreplay.py); HRFD_REF_REPLAY=1
    takes them even where oracle/_ref exists, HRFD_REF_RECORD=1 records them anew
    (tests/golden/make_golden_ref_calls.py)."""
    from tests import reflib, refreplay
    if os.environ.get("HRFD_REF_REPLAY") == "1" and refreplay.have_recording():
        yield refreplay.player(reflib.Oracle())
        return
    if not reflib.have_ref():
        if os.path.isdir("/root/reference/radioDiags"):
            import subprocess
            subprocess.check_call(["make", "-C", reflib.ORACLE_DIR, "ref"], stdout=subprocess.DEVNULL)
        elif refreplay.have_recording():
            yield refreplay.player(reflib.Oracle())
            return
        else:
            pytest.skip("oracle/_ref not built and /root/reference absent")
    if os.environ.get("HRFD_REF_RECORD") == "1":
        rec = refreplay.recorder(reflib.Ref(), reflib.Oracle())
        yield rec
        rec.save()
        return
    yield reflib.Ref()


@pytest.fixture(autouse=True)
def _ref_calls_of_this_test(request):
    """the recorded answers of the reference are kept per test (tests/refreplay.py)"""
    if "ref" in request.fixturenames:
        from tests import refreplay
        key = f"{os.path.basename(str(request.node.fspath))}::{request.node.name}"
        if isinstance(request.getfixturevalue("ref"), refreplay.Player) and key not in refreplay.SESSION.calls:
            pytest.skip("oracle/_ref not built, and no recorded answers of the reference for this test")
        refreplay.SESSION.begin(key)
        yield
        refreplay.SESSION.finish()
        return
    yield


# the behaviour-changing hooks of include/hrfd_debug.h as the Python binding spells them
GATED_HOOKS = ("debug_set_atan", "debug_set_warm", "debug_set_run_len", "debug_set_stream", "debug_expire", "debug_set_fir_flow",
               "debug_set_gated", "debug_set_stagger", "debug_set_sliced", "debug_set_scan", "debug_set_tail")


@pytest.fixture(autouse=True, scope="session")
def _skip_what_needs_a_hook_when_the_hooks_are_off():
    """HRFD_HOOKS_OFF=1: a test that reaches for a behaviour-changing hook skips there (tests where the hook is an extra
    -- a second kernel over the same input -- ask tests.hooks.HOOKS_ON and leave it out instead)."""
    from tests.hooks import HOOKS_ON
    if not HOOKS_ON:
        from hackrfdiags_amd import api
        for cls in (api.Rx, api.Mod, api.Demod):
            for name in GATED_HOOKS:
                if hasattr(cls, name):
                    def refuse(self, *a, _n=name, **kw):
                        pytest.skip(f"{_n} needs HRFD_DEBUG_HOOKS=1 (this run is the shipped state)")
                    setattr(cls, name, refuse)
    yield

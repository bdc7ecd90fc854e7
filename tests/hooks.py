"""Is this process one that asked libhrfd for its behaviour-changing test hooks?  (tests/conftest.py sets
HRFD_DEBUG_HOOKS=1 unless HRFD_HOOKS_OFF=1: the shipped state, run by tests/test_gpu_hooks_off.py in a child process.)"""
import os
import subprocess
import sys

HOOKS_ON = os.environ.get("HRFD_DEBUG_HOOKS") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def answers_without_and_with_the_opt_in(call):
    """`call`, the text of a call on L (the loaded library), in two fresh processes: one started without HRFD_DEBUG_HOOKS
    and one with HRFD_DEBUG_HOOKS=1 (libhrfd reads the variable once per process).  Returns what each printed:
    "<return code> <hrfd_last_error()>".  Needs no GPU."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from hackrfdiags_amd import _lib\n"
            "L = _lib.load()\n"
            "print(%s, L.hrfd_last_error().decode())\n" % (ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "HRFD_DEBUG_HOOKS"}
    off = subprocess.check_output([sys.executable, "-c", code], env=env, text=True)
    on = subprocess.check_output([sys.executable, "-c", code], env={**env, "HRFD_DEBUG_HOOKS": "1"}, text=True)
    return off, on


def check_max_wgs_hook_refusals(name):
    """hrfd_<bank>_debug_set_max_wgs changes how a call is cut into launches, so it answers HRFD_ESTATE (-4, naming the
    variable) in a process that did not start with HRFD_DEBUG_HOOKS=1, before it looks at its arguments: a valid and an
    invalid count get the same answer.  With the opt-in it refuses the NULL handle with HRFD_EINVAL (-1)."""
    for n in (1, 0):
        off, on = answers_without_and_with_the_opt_in(f"L.{name}(None, {n})")
        assert off.startswith(f"-4 {name}") and "HRFD_DEBUG_HOOKS" in off, off
        assert on.startswith(f"-1 {name}") and "handle" in on, on

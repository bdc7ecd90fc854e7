"""Records tests/golden/ref_calls.pkl.xz: every answer the reference's own compiled sources (oracle/_ref, built by
oracle/Makefile where the reference tree exists) give to the CPU tests that question them through the `ref` fixture --
a digest where the oracle's answer to the same call was the same, the answer itself where it was not.
Where oracle/_ref cannot be built, the fixture serves these answers back (tests/refreplay.py).

    python tests/golden/make_golden_ref_calls.py          (needs oracle/_ref: `make -C oracle ref`)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MODULES = ["tests/test_oracle_vs_ref.py", "tests/test_short_blocks.py", "tests/test_txring.py"]

if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from tests import reflib
    if not reflib.have_ref():
        raise SystemExit("oracle/_ref is not built: nothing to record")
    env = dict(os.environ, HRFD_REF_RECORD="1")
    env.pop("HRFD_REF_REPLAY", None)
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu"] + MODULES,
                          cwd=ROOT, env=env)

#!/usr/bin/env python3
"""Records tests/golden/ref_runs/: what the reference's binaries (oracle/_ref, make -C oracle ref) print -- and the index
files they write -- for the runs of the tests that compare with them directly.  Where oracle/_ref is not built those tests
replay these records (tests/oracle_bind.py: keyed by binary, argv and the bytes of the input files).

    python tests/golden/make_ref_runs.py
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import oracle_bind  # noqa: E402

TESTS = ["tests/test_oracle_vs_ref.py",
         "tests/test_sdust.py::test_oracle_sdust_vs_reference_binary_on_synthetic_reads",
         "tests/test_emu_pipeline.py::test_fuzz_tool_runs_a_case",
         "tests/test_intervals.py::test_interval_inputs_have_teeth"]


def main():
    if not (oracle_bind.have_ref() and os.path.exists(oracle_bind.REF_SDUST)):
        raise SystemExit("oracle/_ref is not built (make -C oracle ref)")
    shutil.rmtree(oracle_bind.RECORDED, ignore_errors=True)
    env = dict(os.environ, LQCOV_RECORD_REF="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env)
    n = len(os.listdir(oracle_bind.RECORDED)) if os.path.isdir(oracle_bind.RECORDED) else 0
    print("%d files in %s" % (n, oracle_bind.RECORDED))
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()

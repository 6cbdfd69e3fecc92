#!/usr/bin/env python3
"""Writes tests/golden/intervals/: the inputs of tests/test_intervals.py as tests.helpers.make_interval_cases generates them --
<name>.txt.gz, the text `ref_harness intervals` reads, and cases.json, what the tests know of each case besides.  The recorded
runs of the reference (tests/golden/ref_runs/, tests/golden/make_ref_runs.py) are keyed by the bytes of these texts: after a
change of the generator, run this and then record again.

    python tests/golden/make_interval_inputs.py
"""
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.helpers import make_interval_cases, write_interval_case  # noqa: E402


def main():
    out = os.path.join(HERE, "intervals")
    os.makedirs(out, exist_ok=True)
    meta = []
    with tempfile.TemporaryDirectory() as d:
        for c in make_interval_cases():
            fn = os.path.join(d, "c.txt")
            write_interval_case(c, fn)
            with open(fn, "rb") as f, open(os.path.join(out, c["name"] + ".txt.gz"), "wb") as g, gzip.GzipFile(fileobj=g, mode="wb", mtime=0) as z:
                z.write(f.read())
            meta.append(dict(name=c["name"], min_cov=c["min_cov"], grows=c["grows"], random=c["random"],
                             quirk={str(q): list(v) for q, v in sorted(c["quirk"].items())}))
    with open(os.path.join(out, "cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("%d cases in %s" % (len(meta), out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What the device sees of the mapping stage, as a listing two builds can be compared by (profiles/README.md, r30_a).

    LQCOV_LIBRARY=<liblqcov.so, or the emulator build of tools/emutrace/hipemu.hpp> python tools/launch_order.py OUT.txt

One job per case, each in a process of its own with LQCOV_LANES=1 LQCOV_TRACE_LAUNCHES=1: the inputs of
test_emulated_observable_ties_scheme under five environments and one case of test_emulated_saturated_counters_are_replayed.
Per case the listing holds the `[lqcov] launch <kernel> grid <g> stream <p>` lines of stderr with every stream pointer replaced
by its order of first appearance, [(stage, launches, bytes)] from stage_times() in profiling mode 2, and the SHA-256 of the
output table.  `diff` of two listings: empty when the builds launch the same kernels in the same order."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("ties", {}), ("ties", {"LQCOV_FILTER": "0"}), ("ties", {"LQCOV_TIES": "klib"}),
         ("ties", {"LQCOV_SEED_SURV_MAX": "1000", "LQCOV_SEED_CHUNK": "4000"}),      # groups and regrouping
         ("ties", {"LQCOV_ANCHOR_BUDGET": "20000"}),                                  # several batches, second-pass subsets
         ("saturated", {"LQCOV_TEST_CNT_BITS": "5"})]


def child(kind):
    import pathlib
    from longqc_amd import api
    from tests import test_emu_pipeline as T
    from tests.helpers import ONT
    with tempfile.TemporaryDirectory() as d:
        if kind == "ties":
            tf, qf = T._repeat_rich_dataset(pathlib.Path(d), 2, n_targets=12, n_queries=2, glen=21000)
            argv = ONT + [tf, qf]
        else:
            tf, qf = T._pileup_dataset(pathlib.Path(d), 300)
            argv = ["-Y", "-l", "0", "-q", "40", "-k", "12", "-w", "5", "-I", "4G", "-p", "40", "-m", "20", "-t", "4", tf, qf]
        p, _, _ = api.parse_args(argv)
        eng = api.Engine(p, 0, lib=api.load_library(os.environ["LQCOV_LIBRARY"]))
        eng.set_profiling(2)
        out = os.path.join(d, "o.tsv")
        eng.run_files(tf, qf, out=out, err=os.path.join(d, "e.log"))
        stages = [(s["name"], s["launches"], s["algo_bytes"]) for s in eng.stage_times()]
        eng.close()
        print(json.dumps(dict(stages=stages, table=hashlib.sha256(open(out, "rb").read()).hexdigest())))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    lines = []
    for kind, env in CASES:
        e = dict(os.environ, LQCOV_LANES="1", LQCOV_TRACE_LAUNCHES="1", **env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            return 1
        head = "== %s %s" % (kind, " ".join("%s=%s" % kv for kv in sorted(env.items())) or "default")
        lines.append(head)
        streams, n = {}, 0
        for ln in r.stderr.splitlines():
            m = re.match(r"\[lqcov\] launch (.*) grid (\d+) stream (\S+)$", ln)
            if m:
                lines.append("%s grid %s stream s%d" % (m.group(1), m.group(2), streams.setdefault(m.group(3), len(streams))))
                n += 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        lines += ["stage %s launches %d bytes %d" % tuple(s) for s in res["stages"]]
        lines.append("table sha256 %s" % res["table"])
        lines.append("launches %d" % n)
        print(head, n, "launches", flush=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The RS-II platform QC (longqc_amd/rs.py) on a synthetic run directory: an sts.csv of N rows and 60 columns (the four that
lq_rs.run_platformqc uses among integers, decimals and text, as an RS-II file has them; a third of the ZMWs empty) and an sts.xml.
Timed, after a start-up call on a small run: run_platformqc, file -> JSON block and figure data, and its parts (the table read,
lengths(), the box statistics).  Beside it, alternated in the same run on the same host where pandas imports: pd.read_table(sep=',')
of the same file plus the reference's statistics restated with numpy (mask, sums, the descending sort for N50 / N90, the two
histograms, the log-sum; no fit, no box plot and no drawing: the reference pays those on top).  The two sides' integers must be equal.
Median (min-max) seconds over --reps; one JSON line per size, also written to $OUT/rs_time.json when OUT is set.
Usage: python tools/rs_time.py [--rows 150000] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import rs  # noqa: E402

XML = """<?xml version="1.0" encoding="utf-8"?>
<PipeStats xmlns="http://pacificbiosciences.com/PipelineStats/PipeStats.xsd">
  <ProdDist><BinCount>1</BinCount><BinCount>2</BinCount><BinCount>3</BinCount><BinLabel>Empty</BinLabel><BinLabel>Productive</BinLabel><BinLabel>Other</BinLabel></ProdDist>
</PipeStats>
"""
N_COLS = 60


def write_run(d, n, seed):
    rng = np.random.default_rng(seed)
    empty = rng.random(n) < 0.33
    length = np.where(empty, 0, rng.gamma(2.0, 7000.0, n).astype(np.int64) + 50)
    start = np.where(empty, 0, rng.integers(0, 400, n))
    bases = start + length + rng.integers(0, 2000, n)
    score = np.where(empty, 0.0, 0.11 + 0.88 * rng.random(n))
    filler = rng.random((n, 8))
    names = ["Zmw", "HoleNumber", "X", "Y", "ZmwType", "HoleStatus", "ReadScore", "NumBases", "HQRegionStart", "HQRegionEnd"]
    names += ["Metric%d" % k for k in range(N_COLS - len(names))]
    with open(os.path.join(d, "m1.sts.csv"), "w") as f:
        f.write(",".join(names) + "\n")
        for i in range(n):
            row = [str(i), str(10000 + i), str(i % 300), str(i // 300), "SEQUENCING", "0", "%.4f" % score[i], str(bases[i]), str(start[i]), str(start[i] + length[i])]
            row += ["%.5f" % filler[i, k % 8] if k % 5 else "FullHqRead%d" % (k % 3) for k in range(N_COLS - len(row))]
            f.write(",".join(row) + "\n")
    with open(os.path.join(d, "m1.sts.xml"), "w") as f:
        f.write(XML)
    return os.path.getsize(os.path.join(d, "m1.sts.csv"))


def pandas_side(d):
    import pandas as pd
    df = pd.read_table(os.path.join(d, "m1.sts.csv"), sep=",")
    t1 = time.perf_counter()
    mask = df["ReadScore"] > 0.1
    vals = df["HQRegionEnd"].values[mask] - df["HQRegionStart"].values[mask]
    nb = df["NumBases"].values[mask]
    desc = np.sort(vals)[::-1]
    cum = np.cumsum(desc)
    out = {"Throughput": int(vals.sum()), "Longest_read": int(vals.max()), "Num_of_reads": int(vals.size), "n50": int(desc[np.argmax(2 * cum >= cum[-1])]),
           "n90": int(desc[np.argmax(100 * cum >= 90 * cum[-1])]), "log_sum": float(np.log(vals).sum()), "fraction": float(np.mean(vals / nb))}
    for x in (vals, nb):
        np.histogram(x, bins=np.arange(x.min(), x.max() + 1000, 1000), density=True)
    return out, t1


def med(ts):
    return {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="150000")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    try:
        import pandas  # noqa: F401
        have_pandas = True
    except ImportError:
        have_pandas = False
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        small = os.path.join(tmp, "small")
        os.makedirs(small)
        write_run(small, 2000, 1)
        rs.run_platformqc(small)                                      # start-up: the library, the context, the first allocations
        if have_pandas:
            pandas_side(small)
        for n in (int(x) for x in a.rows.split(",")):
            d = os.path.join(tmp, "run%d" % n)
            os.makedirs(d)
            size = write_run(d, n, 7)
            t_run, t_read, t_len, t_box, t_pd, t_pd_read = [], [], [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                js, fig = rs.run_platformqc(d)
                t_run.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                with rs.StsTable(os.path.join(d, "m1.sts.csv")) as t:
                    t1 = time.perf_counter()
                    t.lengths()
                    t2 = time.perf_counter()
                    t.box_stats("ReadScore", 1000)
                    t3 = time.perf_counter()
                    stats = dict(t.stats)
                t_read.append(t1 - t0); t_len.append(t2 - t1); t_box.append(t3 - t2)
                if have_pandas:
                    t0 = time.perf_counter()
                    ref, t1 = pandas_side(d)
                    t_pd.append(time.perf_counter() - t0); t_pd_read.append(t1 - t0)
                    got = {"Throughput": js["Throughput"], "Longest_read": js["Longest_read"], "Num_of_reads": js["Num_of_reads"], "n50": int(fig["n50"]), "n90": int(fig["n90"])}
                    assert got == {k: ref[k] for k in got}, (got, ref)
            line = {"rows": n, "columns": N_COLS, "file_bytes": size, "reps": a.reps, "stats": stats, "run_platformqc": med(t_run), "table_read": med(t_read),
                    "lengths": med(t_len), "box_stats": med(t_box), "pandas_read_table_plus_numpy": med(t_pd) if t_pd else None,
                    "pandas_read_table_alone": med(t_pd_read) if t_pd_read else None}
            print(json.dumps(line))
            lines.append(line)
    if os.environ.get("OUT"):
        with open(os.path.join(os.environ["OUT"], "rs_time.json"), "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The per-read figure data of a whole run (longqc_amd/figdata.py: box_stats and masked_fraction_hist, what lq_mask.py:43-79 computes over
every read before it draws) on arrays of configs[1]'s and configs[2]'s read counts: 50k and 500k synthetic reads -- gamma-distributed
lengths, a mean QV per read around 10 with one read in fifty without qualities, a masked fraction per read -- as the integer thousandths
the pass keeps.  Beside it the reference's own operations on the same arrays on the same host in the same run: np.floor(len / 3000),
pandas' groupby and matplotlib.cbook.boxplot_stats per bin where both import (else np.percentile and the whisker rules in numpy), and
np.histogram(fractions, np.arange(0, 1.0, 0.01)).  A call on small arrays first takes the device's start-up out of the figures; then
three alternated repetitions, reported as median (min-max) seconds; box_stats_raw (the device call without the host's assembly of the
fliers) is timed on its own before box_stats in every repetition and so meets the cold buffers.  The two sides' numbers must be equal.
With LQCOV_TIMING=1 the library prints each lqfig_boxstats call's stages (allocation, upload, sort, the other kernels, download) on
stderr; the waits that close the stages then count into the figures above, so take the stages from a run of their own.  One JSON line per size (also written to $OUT/boxstats_time.json when OUT is set).
Usage: python tools/boxstats_time.py [--sizes cfg2,cfg3] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import figdata  # noqa: E402

SIZES = {"cfg2": ("configs[1]", 50000, 15000, 1.6), "cfg3": ("configs[2]", 500000, 10000, 2.0)}
MISSING = figdata.MISSING


def make_arrays(n_reads, mean_len, shape, seed):
    rng = np.random.default_rng(seed)
    lens = np.maximum(50, rng.gamma(shape, mean_len / shape, n_reads)).astype(np.uint32)
    qv = np.round(1000 * np.clip(10 + 2.5 * rng.standard_normal(n_reads), 0, 40)).astype(np.int32)
    qv[rng.integers(0, n_reads, n_reads // 50)] = MISSING
    frac = np.round(1000 * np.clip(rng.beta(1.2, 20, n_reads), 0, 1)).astype(np.uint32)
    return lens, qv, frac


def reference(lens, qv, frac, interval=3000.0):
    """-> ({bin: the box}, the histogram's counts, seconds per operation, which box code ran)"""
    t = {}
    t0 = time.time()
    v = np.where(qv == MISSING, np.nan, qv / 1000)
    bins = np.floor(lens / interval)
    try:
        import pandas as pd
        from matplotlib import cbook
        how = "pandas groupby + cbook.boxplot_stats"
        groups = [(g, sub.dropna().values) for g, sub in pd.DataFrame({"g": bins, "v": v}).groupby("g")["v"]]
        boxes = {int(g): cbook.boxplot_stats(x, whis=1.5)[0] for g, x in groups if x.shape[0]}
    except ImportError:
        how = "numpy restatement"
        order = np.argsort(bins, kind="stable")
        cuts = np.flatnonzero(np.diff(bins[order])) + 1
        boxes = {}
        for x, g in zip(np.split(v[order], cuts), bins[order][np.concatenate([[0], cuts])]):
            x = x[~np.isnan(x)]
            if not x.shape[0]:
                continue
            q1, med, q3 = np.percentile(x, [25, 50, 75])
            hi, lo = x[x <= q3 + 1.5 * (q3 - q1)], x[x >= q1 - 1.5 * (q3 - q1)]
            whishi = q3 if hi.shape[0] == 0 or hi.max() < q3 else hi.max()
            whislo = q1 if lo.shape[0] == 0 or lo.min() > q1 else lo.min()
            boxes[int(g)] = {"q1": q1, "med": med, "q3": q3, "whislo": whislo, "whishi": whishi, "fliers": np.concatenate([x[x < whislo], x[x > whishi]])}
    t["floor_groupby_boxplot_stats_s"] = time.time() - t0
    t0 = time.time()
    counts = np.histogram(frac / 1000, bins=np.arange(0, 1.0, 0.01))[0]
    t["np_histogram_s"] = time.time() - t0
    return boxes, counts, t, how


def spread(vals):
    return "%.4f (%.4f-%.4f)" % (statistics.median(vals), min(vals), max(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lines = []
    lens, qv, frac = make_arrays(2000, 8000, 1.5, 1)                                          # device start-up
    figdata.box_stats(lens, qv, 3000.0); figdata.masked_fraction_hist(frac)
    for name in a.sizes.split(","):
        label, n_reads, mean_len, shape = SIZES[name]
        lens, qv, frac = make_arrays(n_reads, mean_len, shape, 100 + n_reads)
        ours, ref_t = {"box_stats_s": [], "box_stats_raw_alone_s": [], "masked_fraction_hist_s": []}, {}
        for _ in range(a.reps):                                                              # alternated: ours, then the reference's
            t0 = time.time()
            figdata.box_stats_raw(lens, qv, 3000.0)
            ours["box_stats_raw_alone_s"].append(time.time() - t0)
            t0 = time.time()
            box = figdata.box_stats(lens, qv, 3000.0)
            ours["box_stats_s"].append(time.time() - t0)
            t0 = time.time()
            edges, counts = figdata.masked_fraction_hist(frac)
            ours["masked_fraction_hist_s"].append(time.time() - t0)
            ref_boxes, ref_counts, t, how = reference(lens, qv, frac)
            for k, v in t.items():
                ref_t.setdefault(k, []).append(v)
        assert counts.tolist() == ref_counts.tolist()
        some = box["n"] > 0
        assert box["group"][some].tolist() == sorted(ref_boxes)
        for j in np.flatnonzero(some):
            r = ref_boxes[int(box["group"][j])]
            assert all(float(box[k][j]) == float(r[k]) for k in ("q1", "med", "q3", "whislo", "whishi")), (int(box["group"][j]), r)
            assert sorted(box["fliers"][j].tolist()) == sorted(np.asarray(r["fliers"]).tolist())
        res = {"metric": "seconds per box_stats() + masked_fraction_hist() call (the numbers behind the QV box plot by length bin and the masked-fraction histogram of a whole run)",
               "unit": "s", "size": "%s's read count" % label, "n_reads": n_reads, "bins": int(box["group"].shape[0]), "reps": a.reps,
               "value": round(statistics.median(ours["box_stats_s"]) + statistics.median(ours["masked_fraction_hist_s"]), 4),
               "device": {k: spread(v) for k, v in ours.items()}, "reference_on_this_host": {k: spread(v) for k, v in ref_t.items()},
               "reference_total_s": round(sum(statistics.median(v) for v in ref_t.values()), 4), "reference_boxes_by": how, "results_equal": True}
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "boxstats_time.json"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The figure data of a whole run (longqc_amd/figdata.py: LqGCMI355X.figure_data and LqMaskMI355X.length_figure_data, what
longQC.py:449,487-488 compute over every read before the report is written) on arrays of configs[1]'s and configs[2]'s sizes: 50k reads
with 1.0 M sampled windows, 500k reads with 6.9 M windows -- synthetic GC fractions (reads: gc / l of a normal cloud, windows: k / 150)
and gamma-distributed lengths of those counts, as float32 / integers like the pass keeps them.  Where scipy is importable, the
reference's own operations on the same arrays on the same host in the same run: scipy.stats.gaussian_kde(x)(xs) twice, np.histogram
twice, scipy.stats.gamma.fit(lens, floc=0) and the length histogram.  A call on small arrays first takes the device's start-up out of
the figures; then three alternated repetitions, reported as median (min-max) seconds, with the host passes inside the two calls timed on
the side (the bandwidth's np.cov over the array, the sort behind summary()'s N50).  The two sides' numbers are compared as well: the
histograms must be equal, the curves and the fit are reported as largest relative differences.  One JSON line per size (also written to
$OUT/figdata_time.json when OUT is set).
Usage: python tools/figdata_time.py [--sizes cfg2,cfg3] [--reps 3]"""
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

from longqc_amd import figdata, gcfrac, sdust  # noqa: E402

SIZES = {"cfg2": ("configs[1]", 50000, 1000000, 15000, 1.6), "cfg3": ("configs[2]", 500000, 6900000, 10000, 2.0)}


def make_arrays(n_reads, n_windows, mean_len, shape, seed):
    rng = np.random.default_rng(seed)
    lens = np.maximum(50, rng.gamma(shape, mean_len / shape, n_reads)).astype(np.int64)
    r = (np.round(lens * np.clip(0.41 + 0.015 * rng.standard_normal(n_reads), 0.05, 0.95)) / lens).astype(np.float32)
    c = (np.round(150 * np.clip(0.41 + 0.045 * rng.standard_normal(n_windows), 0, 1)) / np.float64(150)).astype(np.float32)
    return r, c, lens


def objects(r, c, lens, work):
    lg = gcfrac.LqGCMI355X()
    lg.r_frac.frombytes(r.tobytes())
    lg.c_frac.frombytes(c.tobytes())
    lm = sdust.LqMaskMI355X(work)
    for k, part in enumerate(np.array_split(lens, 8)):
        lm._note(k, part, 0, 0, [], [])
    return lg, lm


def reference(r, c, lens, b_width=0.02):
    """what plot_unmasked_gc_frac and longQC.py:487-488 compute before they draw -> (the numbers, seconds per operation)"""
    from scipy.stats import gamma, gaussian_kde
    xs = np.linspace(0, 1.0, 50)
    out, t = {}, {}
    t0 = time.time()
    out["read_hist"] = np.histogram(r, bins=np.arange(float(r.min()), float(r.max()) + b_width, b_width), density=True)
    out["chunk_hist"] = np.histogram(c, bins=np.arange(float(c.min()), float(c.max()) + b_width, b_width), density=True)
    t["np_histogram_x2_s"] = time.time() - t0
    t0 = time.time()
    out["read_kde"] = gaussian_kde(r)(xs)
    t["gaussian_kde_reads_s"] = time.time() - t0
    t0 = time.time()
    out["chunk_kde"] = gaussian_kde(c)(xs)
    t["gaussian_kde_windows_s"] = time.time() - t0
    t0 = time.time()
    a, _, scale = gamma.fit(lens, floc=0.0)
    out["gamma_params"] = (a, scale)
    t["gamma_fit_s"] = time.time() - t0
    t0 = time.time()
    out["length_hist"] = np.histogram(lens, bins=np.arange(int(lens.min()), int(lens.max()) + 1000, 1000), density=True)
    t["length_histogram_s"] = time.time() - t0
    return out, t


def timed_parts(fn, parts):
    """fn() with the host passes inside it timed on the side: figdata.scott_bandwidth (np.cov over the array) and the mask's summary()
    (the sort behind N50) -> (result, wall, {part: seconds})"""
    spent = {k: 0.0 for k in parts}
    real = {"bandwidth_s": figdata.scott_bandwidth, "summary_s": sdust.LqMaskMI355X.summary}

    def wrap(f, key):
        def g(*a, **kw):
            t = time.time()
            out = f(*a, **kw)
            spent[key] += time.time() - t
            return out
        return g
    if "bandwidth_s" in parts:
        figdata.scott_bandwidth = wrap(real["bandwidth_s"], "bandwidth_s")
    if "summary_s" in parts:
        sdust.LqMaskMI355X.summary = wrap(real["summary_s"], "summary_s")
    try:
        t0 = time.time()
        out = fn()
        wall = time.time() - t0
    finally:
        figdata.scott_bandwidth, sdust.LqMaskMI355X.summary = real["bandwidth_s"], real["summary_s"]
    return out, wall, spent


def spread(vals):
    return "%.4f (%.4f-%.4f)" % (statistics.median(vals), min(vals), max(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    try:
        import scipy
        have_scipy = scipy.__version__
    except ImportError:
        have_scipy = None
    lines = []
    with tempfile.TemporaryDirectory() as work:
        lg, lm = objects(*make_arrays(2000, 20000, 8000, 1.5, 1), work)                       # device start-up
        lg.figure_data(); lm.length_figure_data()
        for name in a.sizes.split(","):
            label, n_reads, n_windows, mean_len, shape = SIZES[name]
            r, c, lens = make_arrays(n_reads, n_windows, mean_len, shape, 100 + n_reads)
            lg, lm = objects(r, c, lens, work)
            lr, lc = np.array(lg.r_frac, dtype=np.float32), np.array(lg.c_frac, dtype=np.float32)
            ours, ref_t, ref = {"figure_data_s": [], "of_it_bandwidth_s": [], "length_figure_data_s": [], "of_it_summary_s": []}, {}, None
            for _ in range(a.reps):                                                              # alternated: ours, then the reference's
                gc, wall, spent = timed_parts(lg.figure_data, ["bandwidth_s"])
                ours["figure_data_s"].append(wall); ours["of_it_bandwidth_s"].append(spent["bandwidth_s"])
                ln, wall, spent = timed_parts(lm.length_figure_data, ["summary_s"])
                ours["length_figure_data_s"].append(wall); ours["of_it_summary_s"].append(spent["summary_s"])
                if have_scipy:
                    ref, t = reference(lr, lc, lens)
                    for k, v in t.items():
                        ref_t.setdefault(k, []).append(v)
            res = {"metric": "seconds per figure_data() + length_figure_data() call (the numbers behind the GC and the length figure of a whole run)",
                   "unit": "s", "size": "%s-sized arrays" % label, "n_reads": n_reads, "n_windows": n_windows, "reps": a.reps,
                   "value": round(statistics.median(ours["figure_data_s"]) + statistics.median(ours["length_figure_data_s"]), 4),
                   "device": {k: spread(v) for k, v in ours.items()}, "bandwidths": [gc["read_bandwidth"], gc["chunk_bandwidth"]],
                   "gamma_params": list(ln["gamma_params"]), "scipy": have_scipy}
            if have_scipy:
                res["reference_on_this_host"] = {k: spread(v) for k, v in ref_t.items()}
                res["reference_total_s"] = round(sum(statistics.median(v) for v in ref_t.values()), 4)
                for key in ("read_hist", "chunk_hist"):
                    assert gc[key][2].tobytes() == ref[key][0].tobytes() and gc[key][0].tobytes() == ref[key][1].tobytes(), key
                assert ln["hist"][2].tobytes() == ref["length_hist"][0].tobytes()
                res["histograms_equal"] = True
                for key in ("read_kde", "chunk_kde"):
                    near = ref[key] >= 1e-6 * ref[key].max()
                    res[key + "_max_rel_diff"] = float(np.max(np.abs(gc[key][near] - ref[key][near]) / ref[key][near]))
                res["gamma_max_rel_diff"] = float(max(abs(x - y) / y for x, y in zip(ln["gamma_params"], ref["gamma_params"])))
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "figdata_time.json"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

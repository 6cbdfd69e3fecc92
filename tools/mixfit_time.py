#!/usr/bin/env python3
"""The coverage estimate of a 5000-row table (covtable.CoverageTable.est_coverage: the two mixture fits of longqc_amd/mixfit.py on the device)
and the batch put to use, bootstrap_main(1000): 1000 refits in one launch.  The table is synthetic -- zeros, a broad background and a main
component, as tests/golden/make_mixfit_golden.py builds its tables -- and a second one of the low-coverage kind takes the log-normal
branch.  Where sklearn is importable, the reference's GaussianMixture(n_components=2).fit of the same selected values on the same host in
the same run, and a loop of `--ref-refits` such fits of resamples for the bootstrap's side.  A call on a small table first takes the
device's start-up out of the figures; then `--reps` alternated repetitions, reported as median (min-max) seconds; the bootstrap's draw and
its one lqmix_gmm2 call are timed again on their own.  One JSON line (also
written to $OUT/mixfit_time.json when OUT is set).  LQCOV_MIXFIT_LIB: another build of the library (the emulator's, to try the tool).
Usage: python tools/mixfit_time.py [--rows 5000] [--nbs 1000] [--reps 9] [--ref-refits 20]"""
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

from longqc_amd import api, mixfit  # noqa: E402
from longqc_amd.covtable import CoverageTable  # noqa: E402


def write_table(path, n, zero_frac, bg_frac, main, sd, seed, lognormal=False, bg_hi=None):
    rng = np.random.default_rng(seed)
    n_zero, n_bg = int(round(n * zero_frac)), int(round(n * bg_frac))
    mainv = np.exp(rng.normal(np.log(main), sd, n - n_zero - n_bg)) if lognormal else rng.normal(main, sd, n - n_zero - n_bg)
    cov = np.concatenate([np.zeros(n_zero), rng.uniform(0.05, bg_hi or 3 * main, n_bg), np.abs(mainv) + 0.001])
    with open(path, "w") as f:
        for i, c in enumerate(cov.tolist()):
            ql = int(rng.integers(400, 20000))
            if c == 0.0:
                f.write("\t".join(["r%d" % i, str(ql), "0", "0", "0", "0.0", "6.500", "0.0", "0.0"]) + "\n")
            else:
                co, text = "%d-%d" % (10, ql - 10), "%.3f" % c
                f.write("\t".join(["r%d" % i, str(ql), str(int(round(c * ql))), co, co, text, "9.250", "0.100", text]) + "\n")
    return path


def spread(vals):
    return "%.5f (%.5f-%.5f)" % (statistics.median(vals), min(vals), max(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--nbs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-refits", type=int, default=20)
    a = ap.parse_args()
    lib = api.load_library(os.environ["LQCOV_MIXFIT_LIB"]) if os.environ.get("LQCOV_MIXFIT_LIB") else None
    try:
        import sklearn
        from sklearn.mixture import GaussianMixture
        have = sklearn.__version__
    except ImportError:
        have = None
    with tempfile.TemporaryDirectory() as d:
        CoverageTable(write_table(os.path.join(d, "warm.txt"), 200, 0.1, 0.2, 20.0, 2.0, 1)).est_coverage(lib=lib).bootstrap_main(8, lib=lib)      # start-up
        plain = CoverageTable(write_table(os.path.join(d, "plain.txt"), a.rows, 0.08, 0.12, 25.0, 2.5, 3))
        low = CoverageTable(write_table(os.path.join(d, "low.txt"), a.rows, 0.35, 0.25, 1.2, 0.6, 21, lognormal=True, bg_hi=6.0))
        t = {"est_coverage_s": [], "est_coverage_lognormal_branch_s": [], "bootstrap_main_s": [], "of_it_the_draw_s": [], "of_it_lqmix_gmm2_s": []}
        ref = {"sklearn_fit_s": [], "sklearn_refit_of_a_resample_s": []}
        for _ in range(a.reps):
            t0 = time.perf_counter(); plain.est_coverage(lib=lib); t["est_coverage_s"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); low.est_coverage(lib=lib); t["est_coverage_lognormal_branch_s"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); boot = plain.bootstrap_main(a.nbs, seed=0, lib=lib); t["bootstrap_main_s"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); samples = plain.selected[np.random.default_rng(0).integers(0, plain.selected.size, size=(a.nbs, plain.selected.size))]
            t["of_it_the_draw_s"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); mixfit.gmm2_raw(list(samples), lib=lib); t["of_it_lqmix_gmm2_s"].append(time.perf_counter() - t0)      # (sorts and split searches on the host inside)
            if have:
                x = plain.selected.reshape(-1, 1)
                t0 = time.perf_counter(); m = GaussianMixture(n_components=2).fit(x); ref["sklearn_fit_s"].append(time.perf_counter() - t0)
                rng = np.random.default_rng(0)
                t0 = time.perf_counter()
                for _k in range(a.ref_refits):
                    GaussianMixture(n_components=2).fit(x[rng.integers(0, x.shape[0], x.shape[0])])
                ref["sklearn_refit_of_a_resample_s"].append((time.perf_counter() - t0) / max(a.ref_refits, 1))
        assert low.mix_model is not None and plain.mix_model is None
        res = {"metric": "seconds per est_coverage() of a %d-row table and per bootstrap_main(%d)" % (a.rows, a.nbs), "unit": "s", "rows": a.rows,
               "selected": int(plain.selected.size), "nbs": a.nbs, "reps": a.reps, "value": round(statistics.median(t["est_coverage_s"]), 5),
               "device": {k: spread(v) for k, v in t.items()}, "gmm_n_iter": plain.model["n_iter"], "lognorm_passes": low.mix_fit["n_iter"],
               "mean": plain.get_mean(), "sd": float(plain.get_sd()), "bootstrap_mean_ci": list(boot["mean_ci"]), "bootstrap_sd_ci": list(boot["sd_ci"]),
               "sklearn": have}
        if have:
            res["reference_on_this_host"] = {k: spread(v) for k, v in ref.items()}
            res["reference_bootstrap_extrapolated_s"] = round(statistics.median(ref["sklearn_refit_of_a_resample_s"]) * a.nbs, 3)
            k = int(np.argmax(m.weights_ / m.covariances_.ravel()))
            res["mean_rel_diff_to_sklearn"] = abs(float(m.means_.ravel()[k]) - plain.get_mean()) / plain.get_mean()
    print(json.dumps(res), flush=True)
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "mixfit_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

"""Writes tests/golden/mixfit_cases.json and the tests/golden/mixfit_*.table.gz it names: seeded synthetic 9-column coverage tables (zeros +
a broad background + a main component) and what LongQC's LqCoverage reports for each of them under 20 seeds (np.random.seed(s) before
LqCoverage(...), the rows permuted by the seed; plot_length_vs_coverage called for its outlier warning): every getter, the Gaussian mixture's n_iter_ / weights / means / covariances, mix_model,
the raw histogram (its edges are np.arange of the recorded mean and sd) and calc_xome_size(1e9); for seed 0 also plot_coverage_dist's curves and, in the file's own
row order, __region_analysis's three lists (whole for the small tables, as counts, sums and the figure's two histograms for the others).  The file
keeps of the 20 records what summary() below says: what all seeds agree on once, every fit-derived number's range over the seeds, the distinct
verdicts and strings, and one seed's own fit and histogram.  And four fixed-start runs of mixEM's normal + log-normal EM
under 4 row permutations, with one more that ends in its NaN exit.  Data only: the reference's lq_coverage.py and mixEM are imported from
the reference tree at generation time, none of their text is written.

Checked while generating, with the numpy model of tests/mixfit_model.py (the deterministic start of longqc_amd/csrc/mixfit.cpp, then
sklearn's E/M steps and stopping rule): every case named "unanimous" is unanimous (all seeds agree to 1e-12 relative with one n_iter_)
and every case named "split" has the model's result inside the seeds' [min, max].

Run with sklearn, pandas, scipy and matplotlib importable:  python tests/golden/make_mixfit_golden.py <LongQC tree>"""
import gzip
import json
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
SEEDS = list(range(20))


def table_rows(seed, n, zero_frac, bg_frac, main, sd, bg_hi=None, lognormal=False, nan_rows=0, long_read_factor=1.0):
    """zeros + a broad background + a main component -> rows of 9 strings"""
    rng = np.random.default_rng(seed)
    n_zero, n_bg = int(round(n * zero_frac)), int(round(n * bg_frac))
    n_main = n - n_zero - n_bg
    bg = rng.uniform(0.05, bg_hi if bg_hi else 3 * main, n_bg)
    mainv = np.exp(rng.normal(np.log(main), sd, n_main)) if lognormal else rng.normal(main, sd, n_main)
    cov = np.concatenate([np.zeros(n_zero), bg, np.abs(mainv) + 0.001])
    rows = []
    for i, c in enumerate(cov.tolist()):
        ql = 800 * int(rng.integers(1, 25))                           # (few distinct digits beside the coverage: the files stay small)
        if c == 0.0:
            rows.append(["r%d" % i, str(ql), str(int(rng.integers(0, 3)) * ql // 1000), "0", "0", "0.0", "%d.500" % rng.integers(4, 9), "0.0", "0.0"])
            continue
        if ql >= 15000 and i >= n_zero + n_bg:
            c *= long_read_factor                                   # (a main component that thins out over the long reads: the outlier warning)
        co = "%d-%d" % (10 * (i % 3), ql - 10)
        text = "%.3f" % c
        rows.append(["r%d" % i, str(ql), str(int(round(c * ql))), co, co, text, "%d.250" % (7 + i % 5), "0.%d00" % (1 + i % 3), text if i >= n_zero + nan_rows else "-nan"])
    return rows


def coords_rows():
    """one, two and unsorted regions in column 3, '0' rows between them"""
    rng = np.random.default_rng(77)
    rows = table_rows(78, 40, 0.2, 0.2, 12.0, 1.5)
    for i, r in enumerate(rows):
        if r[3] == "0":
            continue
        ql = int(r[1])
        if i % 3 == 0:
            m = ql // 2
            r[3] = "%d-%d,%d-%d" % (int(rng.integers(0, 100)), m - 30, m + 40, ql - int(rng.integers(0, 100)))
        elif i % 3 == 1:
            t = ql // 3
            r[3] = "%d-%d,%d-%d,%d-%d" % (2 * t + 10, ql - 7, 5 + i, t - 20, t + 15, 2 * t - 11)          # unsorted: the last region first
    return rows


TABLES = [
    # name, expected kind (None: recorded as it comes), transcript, rows
    ("unanimous_400", "unanimous", False, lambda: table_rows(1, 400, 0.1, 0.15, 30.0, 3.0)),
    ("unanimous_5000", "unanimous", False, lambda: table_rows(3, 5000, 0.08, 0.12, 25.0, 2.5)),
    ("split_a", "split", False, lambda: table_rows(11, 300, 0.1, 0.3, 20.0, 4.0)),
    ("split_b", "split", False, lambda: table_rows(12, 700, 0.05, 0.35, 15.0, 3.5)),
    ("split_c", "split", False, lambda: table_rows(13, 1200, 0.1, 0.4, 28.0, 6.0)),
    ("low_coverage", None, False, lambda: table_rows(21, 600, 0.35, 0.25, 1.2, 0.6, bg_hi=6.0, lognormal=True)),
    ("transcript", None, True, lambda: table_rows(22, 500, 0.1, 0.2, 9.0, 0.5, lognormal=True)),
    ("mostly_zeros", None, False, lambda: table_rows(23, 400, 0.88, 0.04, 14.0, 1.5)),
    ("all_zero", None, False, lambda: table_rows(24, 60, 1.0, 0.0, 10.0, 1.0)),
    ("nan_coverages", None, False, lambda: table_rows(25, 300, 0.1, 0.15, 22.0, 2.5, nan_rows=9)),
    ("many_unmapped", None, False, lambda: table_rows(26, 500, 0.45, 0.1, 33.0, 3.0)),
    ("coords", None, False, coords_rows),
    ("length_bias", None, False, lambda: table_rows(27, 1200, 0.05, 0.1, 30.0, 2.0, long_read_factor=0.5)),
]


def flo(v):
    return None if v is None else float(v)


def record(lc, hist, throughput=1e9):
    m = lc.model
    with tempfile.TemporaryDirectory() as d:                        # (the outlier check runs inside this plot: its warning is recorded below)
        lc.plot_length_vs_coverage(os.path.join(d, "cl.png"))
    rec = {"mean": flo(lc.get_mean()), "sd": flo(lc.get_sd()), "logn_mode": flo(lc.get_logn_mode()), "logn_mu": flo(lc.get_logn_mu()),
           "logn_sigma": flo(lc.get_logn_sigma()), "expected_zero_rate": [flo(v) for v in lc.get_expected_zero_rate()],
           "unmapped_frac": lc.get_unmapped_frac(), "unmapped_med_frac": lc.get_unmapped_med_frac(), "high_div_frac": lc.get_high_div_frac(),
           "no_coverage": lc.is_no_coverage(), "low_coverage": None if lc.is_low_coverage() is None else bool(lc.is_low_coverage()),
           "min_lambda": lc.min_lambda, "max_lambda": lc.max_lambda, "warnings": lc.get_warnings(), "errors": lc.get_errors(),
           "xome": lc.calc_xome_size(throughput), "raw_hist": [float(v) for v in hist[0]]}
    if m is not None:
        o = np.argsort(m.means_.ravel())
        rec["gmm"] = {"n_iter": int(m.n_iter_), "w": m.weights_[o].tolist(), "mu": m.means_.ravel()[o].tolist(), "var": m.covariances_.ravel()[o].tolist(),
                      "lower_bound": float(m.lower_bound_)}
    if lc.mix_model is not None:
        rec["mix_model"] = {"w": [float(v) for v in lc.mix_model[0]], "mu": [float(v) for v in lc.mix_model[1]], "sigma": [float(v) for v in lc.mix_model[2]]}
    return rec


def summary(case, recs, hists):
    """what the tests read of the 20 records: the fields every seed agrees on, the range over the seeds of every number that follows the
    fit, the distinct verdicts / warnings / Xome strings, and seed 0 (and the first seed that differs from it) with its own fit and raw histogram"""
    same = ("unmapped_frac", "unmapped_med_frac", "high_div_frac", "no_coverage", "min_lambda", "max_lambda", "errors")
    assert all(r[k] == recs[0][k] for r in recs for k in same) and len({"mix_model" in r for r in recs}) == 1
    distinct = lambda key: [v for i, v in enumerate([r[key] for r in recs]) if v not in [q[key] for q in recs[:i]]]
    rng = {k: [min(r[k] for r in recs), max(r[k] for r in recs)] for k in ("mean", "sd", "logn_mode", "logn_mu", "logn_sigma") if recs[0][k] is not None}
    rng["zero_rate"] = [min(r["expected_zero_rate"][1] for r in recs), max(r["expected_zero_rate"][1] for r in recs)]
    if "mix_model" in recs[0]:
        rng["logn_w"] = [[min(r["mix_model"]["w"][k] for r in recs) for k in (0, 1)], [max(r["mix_model"]["w"][k] for r in recs) for k in (0, 1)]]
    case.update({"common": {k: recs[0][k] for k in same}, "range": rng, "mix_model": "mix_model" in recs[0], "low_coverage": distinct("low_coverage"),
                 "warnings": distinct("warnings"), "xome": distinct("xome"), "seed_fits": {}})
    if "gmm" in recs[0]:
        case["gmm_range"] = {k: [v.tolist() for v in spread(recs, ("gmm", k))] for k in ("w", "mu", "var")}
    h0 = hists[recs[0]["raw_hist"]]
    other = [s for s, r in enumerate(recs) if len(hists[r["raw_hist"]]) != len(h0) or not np.allclose(hists[r["raw_hist"]], h0, rtol=1e-9, atol=0, equal_nan=True)]
    for s in [0] + other[:1]:                                       # (seed 0, and the first seed whose histogram is another one beyond rounding: the split cases)
        r = recs[s]
        case["seed_fits"][str(s)] = {"mean": r["mean"], "gmm": r.get("gmm"), "mix_model": r.get("mix_model"), "raw_hist": hists[r["raw_hist"]]}


def spread(recs, path):
    vals = np.array([[r[path[0]][path[1]][k] for k in (0, 1)] for r in recs])
    return vals.min(axis=0), vals.max(axis=0)


def main(ref):
    sys.path.insert(0, ref)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import pandas
    import scipy
    import sklearn
    import lq_coverage
    from mixEM import mixem
    from longqc_amd.covtable import CoverageTable
    from tests import mixfit_model as MM
    warnings.simplefilter("ignore")
    seen = []
    plain_hist = plt.hist
    plt.hist = lambda *a, **k: seen.append(plain_hist(*a, **k)) or seen[-1]
    drawn = []
    plain_plot = plt.plot
    plt.plot = lambda *a, **k: drawn.append((np.asarray(a[0]), np.asarray(a[1]))) or plain_plot(*a, **k)
    out = {"versions": {"sklearn": sklearn.__version__, "numpy": np.__version__, "pandas": pandas.__version__, "scipy": scipy.__version__},
           "seeds": SEEDS, "tables": [], "lognorm": []}
    for name, kind, transcript, make in TABLES:
        rows = make()
        fn = "mixfit_%s.table.gz" % name
        text = "".join("\t".join(r) + "\n" for r in rows)
        with gzip.GzipFile(os.path.join(HERE, fn), "wb", mtime=0) as f:
            f.write(text.encode())
        recs = []
        with tempfile.TemporaryDirectory() as d:
            for s in SEEDS:
                p = os.path.join(d, "t%d.txt" % s)
                order = np.random.RandomState(s).permutation(len(rows))
                with open(p, "w") as f:
                    f.write("".join("\t".join(rows[i]) + "\n" for i in order))
                np.random.seed(s)
                del seen[:]
                lc = lq_coverage.LqCoverage(p, isTranscript=transcript)
                rec = record(lc, seen[0])
                if s == 0:
                    del drawn[:]                                    # plot_coverage_dist: the two Poisson curves where the lambdas exist, then the fitted curve
                    lc.plot_coverage_dist(os.path.join(d, "cv.png"))
                    curve = {"poisson": [drawn[0][1].tolist(), drawn[1][1].tolist()] if lc.min_lambda else None,
                             "y_every_500th": drawn[-1][1][::500].tolist() + [float(drawn[-1][1][-1])] if lc.model is not None else None}
                    with open(p, "w") as f:                         # (the three lists follow the rows' order: the file's own order)
                        f.write(text)
                    t5, t3, il = lq_coverage.LqCoverage(p, isTranscript=transcript)._LqCoverage__region_analysis(3, 1)
                    edges = np.arange(0, 145, 5)
                    region = {"n": len(t5), "sum5": int(sum(t5)), "sum3": int(sum(t3)), "n_internal": len(il), "sum_internal": int(sum(il)),
                              "hist5": np.histogram(t5, bins=edges)[0].tolist(), "hist3": np.histogram(t3, bins=edges)[0].tolist()}
                    if len(rows) <= 100:                            # (two numbers per row: the small tables carry the lists themselves)
                        region.update({"t5": [int(v) for v in t5], "t3": [int(v) for v in t3], "internal": [int(v) for v in il]})
                recs.append(rec)
        hists = []                                                  # the distinct histograms once, per seed the place in that list
        for r in recs:
            if r["raw_hist"] not in hists:
                hists.append(r["raw_hist"])
            r["raw_hist"] = hists.index(r["raw_hist"])
        case = {"name": name, "file": fn, "rows": len(rows), "transcript": transcript, "region": region, "curve": curve}
        summary(case, recs, hists)
        if "gmm" in recs[0]:
            iters = sorted({r["gmm"]["n_iter"] for r in recs})
            rel = 0.0
            for key in ("w", "mu", "var"):
                lo, hi = spread(recs, ("gmm", key))
                rel = max(rel, float(((hi - lo) / np.abs(hi)).max()))
            got = "unanimous" if rel <= 1e-12 and len(iters) == 1 else "split"
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "t.txt")
                open(p, "w").write(text)
                model = MM.gmm2(CoverageTable(p).selected_coverage())
            inside = all((spread(recs, ("gmm", key))[0] <= model[key]).all() and (model[key] <= spread(recs, ("gmm", key))[1]).all() for key in ("w", "mu", "var"))
            near = all(np.allclose(model[key], recs[0]["gmm"][key], rtol=1e-9, atol=0) for key in ("w", "mu", "var"))
            print("%-16s %-9s iters %s spread %.2e model n_iter %d inside %s near %s n %d" % (name, got, iters, rel, model["n_iter"], inside, near, model["n"]))
            case.update({"kind": got, "n_iters": iters, "selected": model["n"]})
            if kind == "unanimous":
                assert got == "unanimous" and near and model["n_iter"] == iters[0], name
            if kind == "split":
                assert got == "split" and inside and model["n_iter"] in iters, name
        else:
            case["kind"] = "no_coverage"
            print("%-16s no coverage" % name)
        out["tables"].append(case)
    plt.hist, plt.plot = plain_hist, plain_plot

    # ---- mixEM from a fixed start ---------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(31)
    logn = []
    for name, n, bg_mu, bg_sd, mu, sg, share, start in (
            ("sixty", 60, 8.0, 5.0, 2.3, 0.35, 0.3, (8.0, 5.0, 2.0, 1.0)),
            ("one_past_a_tile", 257, 4.0, 2.5, 3.0, 0.25, 0.2, (4.0, 2.5, 3.2, 1.0)),
            ("four_hundred", 400, 10.0, 6.0, 1.0, 0.6, 0.4, (10.0, 6.0, 1.2, 1.0)),
            ("seven_hundred", 700, 15.0, 8.0, 3.4, 0.2, 0.25, (15.0, 8.0, 3.0, 1.0))):
        nb = int(n * share)
        x = np.concatenate([np.abs(rng.normal(bg_mu, bg_sd, nb)) + 0.001, np.exp(rng.normal(mu, sg, n - nb))])
        logn.append((name, np.round(x, 3) + 0.0, start))
    logn.append(("nan_exit", np.array([1.0, 1.5, 2.0, 2.5, 1e6]), (2.0, 0.5, 0.5, 0.1)))
    for name, x, start in logn:
        runs = []
        for s in range(4):
            xs = x if s == 0 else x[np.random.RandomState(s).permutation(x.size)]
            w, dist, ll = mixem.em(xs, [mixem.distribution.NormalDistribution(start[0], start[1]), mixem.distribution.LogNormalDistribution(start[2], start[3])],
                                   max_iterations=500, progress_callback=None)
            runs.append({"w": [float(v) for v in w], "mu": [float(d.get_mu()) for d in dist], "sigma": [float(d.get_sigma()) for d in dist]})
        model = MM.lognorm_norm(x, start)
        print("%-16s n %d model n_iter %d exit %s ll %r mixem %r" % (name, x.size, model["n_iter"], model["exit"], model["ll"], float(ll)))
        assert (model["exit"] == "nan") == (name == "nan_exit")
        if name != "nan_exit":
            assert all(np.allclose(model[k], runs[0][k], rtol=1e-9, atol=0) for k in ("w", "mu", "sigma"))
        thou = np.sort(np.array([int(round(v * 1000)) for v in x.tolist()], dtype=np.int64))      # (ascending, as steps from one to the next)
        out["lognorm"].append({"name": name, "x_thou_steps": np.diff(thou, prepend=0).tolist(), "start": list(start), "exit": model["exit"],
                               "n_iter": model["n_iter"], "runs": runs})
    dump = lambda v: json.dumps(v, separators=(",", ":"), allow_nan=True)
    with open(os.path.join(HERE, "mixfit_cases.json"), "w") as f:  # (one case per line)
        f.write('{"versions":%s,"seeds":%s,\n"tables":[\n%s],\n"lognorm":[\n%s]}\n' % (dump(out["versions"]), dump(out["seeds"]),
                ",\n".join(dump(c) for c in out["tables"]), ",\n".join(dump(c) for c in out["lognorm"])))
    kinds = [c["kind"] for c in out["tables"]]
    assert kinds.count("unanimous") >= 2 and kinds.count("split") >= 3, kinds
    print("wrote mixfit_cases.json: %d tables (%s), %d log-normal cases" % (len(kinds), ", ".join(sorted(set(kinds))), len(out["lognorm"])))


if __name__ == "__main__":
    main(sys.argv[1])

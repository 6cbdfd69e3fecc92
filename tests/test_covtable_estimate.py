"""CoverageTable's coverage estimate (covtable.est_coverage and what reports it) on the golden tables of tests/golden/mixfit_cases.json, which
hold what LongQC's LqCoverage gave for each table under 20 seeds: under the wave emulator, and on the GPU for the fits' path.

Fit-derived numbers (get_mean, get_sd, the log-normal's mode / mu / sigma, the expected zero rate, the crude Xome size) use the tolerances of
tests/test_mixfit.py 2 and 3: in a unanimous case within max(8 w, r) of the seeds' range, w the recorded width over the seeds; in a split
case inside the seeds' [min, max] widened by r; r = (iterations made) n 2^-53 |v|.  The crude Xome size is an int(...) of a quotient: its
first number lies in the seeds' range widened by 1, the rest of the string is no matter of the fit and equal.  Exact: the fractions, the
verdicts wherever all seeds agree, the lambdas, the raw histogram and the curves of coverage_dist_data() computed from a seed's own fit (to 1e-12), terminal_data(), the
warning of the outlier check, the keys of json_block."""
import gzip
import json
import math
import os

import numpy as np
import pytest

from longqc_amd import api
from longqc_amd import mixfit as M
from longqc_amd.covtable import CoverageTable
from tests.conftest import GOLDEN

U = 2.0 ** -53
CASES = json.load(open(os.path.join(GOLDEN, "mixfit_cases.json")))
NAMES = [c["name"] for c in CASES["tables"]]
BY_NAME = {c["name"]: c for c in CASES["tables"]}


@pytest.fixture(scope="module")
def table_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("mixfit_tables")
    out = {}
    for c in CASES["tables"]:
        out[c["name"]] = str(d / (c["name"] + ".txt"))
        with open(out[c["name"]], "wb") as f:
            f.write(gzip.open(os.path.join(GOLDEN, c["file"])).read())
    return out


def estimates(paths, lib):
    return {nm: CoverageTable(paths[nm]).est_coverage(BY_NAME[nm]["transcript"], lib=lib) for nm in NAMES}


@pytest.fixture(scope="module")
def emu_estimates(table_paths, emu_lib):
    return estimates(table_paths, emu_lib)


def assert_in_range(case, what, got, seen, r):
    """the tolerance of the module's docstring for one fit-derived number; seen: the seeds' values"""
    lo, hi = min(seen), max(seen)
    slack = max(8 * (hi - lo), r * abs(got)) if case["kind"] == "unanimous" else r * abs(got)
    out = max(lo - got, got - hi)
    print("%s %s: %r, the seeds' range [%r, %r], outside by %.3g, allowed %.3g" % (case["name"], what, got, lo, hi, max(out, 0.0), slack))
    assert out <= slack, (case["name"], what, got, lo, hi, slack)


def check_estimate(case, t):
    rng = case["range"]
    for key, got in (("unmapped_frac", t.get_unmapped_frac()), ("unmapped_med_frac", t.get_unmapped_med_frac()), ("high_div_frac", t.get_high_div_frac()),
                     ("min_lambda", t.min_lambda), ("max_lambda", t.max_lambda), ("no_coverage", t.is_no_coverage()), ("errors", t.get_errors())):
        assert case["common"][key] == got, (case["name"], key, got, case["common"][key])
    if len(case["low_coverage"]) == 1:                             # (all seeds agree)
        assert t.is_low_coverage() == case["low_coverage"][0], case["name"]
    if case["kind"] == "no_coverage":
        assert t.model is None and t.get_mean() == 1 and t.get_sd() == math.sqrt(10) and t.calc_xome_size(1e9) == "N/A" and t.get_logn_mode() is None
        assert t.json_block(1e9)["Mean_coverage"] == "NA"
        return
    n = t.selected.size
    assert n == case["selected"] and t.model["n_iter"] in case["n_iters"]
    iters = t.model["n_iter"] + (t.mix_fit["n_iter"] if t.mix_model is not None else 0)
    r = iters * n * U
    assert_in_range(case, "mean", t.get_mean(), rng["mean"], r)
    assert_in_range(case, "sd", float(t.get_sd()), rng["sd"], r)
    assert_in_range(case, "zero rate", t.get_expected_zero_rate()[1], rng["zero_rate"], r * max(1.0, abs(math.log(0.64086)) * t.get_expected_zero_rate()[0]))
    assert (t.mix_model is not None) == case["mix_model"]
    if t.mix_model is not None:
        for key, got in (("logn_mode", t.get_logn_mode()), ("logn_mu", t.get_logn_mu()), ("logn_sigma", t.get_logn_sigma())):
            assert_in_range(case, key, float(got), rng[key], r * (3 if key == "logn_mode" else 1))
        for k in (0, 1):
            assert_in_range(case, "log-normal fit's weight %d" % k, float(t.mix_model[0][k]), [rng["logn_w"][0][k], rng["logn_w"][1][k]], r)
        assert t.get_expected_zero_rate()[0] == t.get_logn_mode()
    else:
        assert t.get_logn_mode() is None and t.get_logn_mu() is None and t.get_logn_sigma() is None
    got, seen = t.calc_xome_size(1e9), case["xome"]
    head, rest = got.split(" ", 1)
    assert rest in {s.split(" ", 1)[1] for s in seen}
    firsts = [int(s.split(" ", 1)[0]) for s in seen]
    assert min(firsts) - 1 <= int(head) <= max(firsts) + 1, (case["name"], got, seen[0])
    block = t.json_block(1e9)
    want = {"Estimated non-sense read fraction", "Estimated crude Xome size"} | ({"Mode_coverage", "mu_coverage", "sigma_coverage"} if (case["transcript"] or t.is_low_coverage())
                                                                              else {"Mean_coverage", "SD_coverage"})
    assert set(block) == want and block["Estimated crude Xome size"] == got and block["Estimated non-sense read fraction"] == case["common"]["unmapped_med_frac"]
    if "Mean_coverage" in block:
        assert block["Mean_coverage"] == t.get_mean() and block["SD_coverage"] == float(t.get_sd())
    else:
        assert block["Mode_coverage"] == float(t.get_logn_mode())
    if case["kind"] == "unanimous":                                # (the edges move with the mean in its last bits: the densities to rounding)
        assert np.allclose(t.raw_hist[0], case["seed_fits"]["0"]["raw_hist"], rtol=1e-9, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_estimate(emu_estimates, name):
    check_estimate(BY_NAME[name], emu_estimates[name])


def test_the_cases_cover_every_branch(emu_estimates):
    t = emu_estimates
    assert t["low_coverage"].is_low_coverage() and t["low_coverage"].min_lambda is None and t["low_coverage"].mix_model is not None
    assert t["mostly_zeros"].is_low_coverage() and t["mostly_zeros"].min_lambda and t["mostly_zeros"].mix_model is not None     # the "edgy case" of :269
    assert t["transcript"].mix_model is not None and not t["transcript"].is_low_coverage()
    assert t["many_unmapped"].min_lambda and t["many_unmapped"].mix_model is None and ", " in t["many_unmapped"].calc_xome_size(1e9)
    assert t["all_zero"].is_no_coverage() and t["all_zero"].is_low_coverage() is None
    assert np.isnan(t["nan_coverages"].cov).sum() == 9 and not np.isnan(t["nan_coverages"].selected).any()
    known = t["mostly_zeros"].cov
    assert np.percentile(known, 85) == 0.0 and t["mostly_zeros"].selected.size == (known != 0).sum() - (known == known.max()).sum()    # quantile(1.0)


def with_the_fit_of(t, case, rec):
    """the table with the reference's own fit of one seed in place of ours: what follows the fit is then a matter of numpy alone"""
    t.model = t.mix_model = None
    t.mean_main, t.cov_main = 1, 10
    t.min_lambda, t.max_lambda = case["common"]["min_lambda"], case["common"]["max_lambda"]
    if rec["gmm"] is not None:
        k = rec["gmm"]["mu"].index(rec["mean"])
        t.model = {key: np.array(rec["gmm"][key]) for key in ("w", "mu", "var")}
        t.mean_main, t.cov_main = rec["mean"], rec["gmm"]["var"][k]
    if rec["mix_model"] is not None:
        t.mix_model = (rec["mix_model"]["w"], rec["mix_model"]["mu"], rec["mix_model"]["sigma"])
    return t


@pytest.mark.parametrize("name", NAMES)
def test_the_raw_histogram_from_a_seeds_own_fit_is_exact(table_paths, name):
    case = BY_NAME[name]
    assert "0" in case["seed_fits"] and (len(case["seed_fits"]) == 2) == (case["kind"] == "split")
    for rec in case["seed_fits"].values():
        density, edges = with_the_fit_of(CoverageTable(table_paths[name]), case, rec)._raw_histogram()
        want = np.array(rec["raw_hist"])
        assert density.shape == want.shape and edges.shape[0] == want.shape[0] + 1
        assert density.tobytes() == want.tobytes() or (np.isnan(want).all() and np.isnan(density).all())


@pytest.mark.parametrize("name", NAMES)
def test_the_curves_from_a_seeds_own_fit_are_the_references(table_paths, name):
    """coverage_dist_data() against what plot_coverage_dist drew for seed 0 (every 500th point of the fitted curve and its last, the two
    Poisson curves whole): the same expressions but scipy.stats' pdf / pmf, each a handful of roundings and one exp of an argument of at most
    ~1e3 in size with its own few units of error: 1e-12 relative, 1e-300 absolute where a curve underflows"""
    case = BY_NAME[name]
    t = with_the_fit_of(CoverageTable(table_paths[name]), case, case["seed_fits"]["0"])
    d, want = t.coverage_dist_data(), case["curve"]
    assert d["x"].shape == (5000,) and d["x"][0] == 0 and d["x"][-1] == t.get_mean() + 10 * t.get_sd() and d["edges"].shape[0] == d["density"].shape[0] + 1
    assert d["density"].tobytes() == np.histogram(t.cov, bins=t._bin_edges(), density=True)[0].tobytes()
    assert d["model"] == (None if case["kind"] == "no_coverage" else "lognorm" if case["mix_model"] else "gmm")
    if want["y_every_500th"] is None:
        assert d["y"] is None
    else:
        assert np.allclose(np.append(d["y"][::500], d["y"][-1]), want["y_every_500th"], rtol=1e-12, atol=1e-300)
    if want["poisson"] is None:
        assert d["poisson"] is None
    else:
        k, lo, hi = d["poisson"]
        assert k.tolist() == list(range(int(t.get_mean() + 4 * t.get_sd()) + 1)) and len(want["poisson"][0]) == k.size
        assert np.allclose(lo, want["poisson"][0], rtol=1e-12, atol=1e-300) and np.allclose(hi, want["poisson"][1], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("name", NAMES)
def test_terminal_data_is_the_references(table_paths, name):
    want, d = BY_NAME[name]["region"], CoverageTable(table_paths[name]).terminal_data()
    assert (len(d["t5"]), sum(d["t5"]), sum(d["t3"]), len(d["internal"]), sum(d["internal"])) == (want["n"], want["sum5"], want["sum3"], want["n_internal"], want["sum_internal"])
    assert len(d["t3"]) == want["n"] and all(isinstance(v, int) for v in d["t5"] + d["t3"] + d["internal"])
    assert d["edges"].tolist() == list(range(0, 145, 5)) and d["hist5"].dtype.kind == "i"
    assert d["hist5"].tolist() == want["hist5"] and d["hist3"].tolist() == want["hist3"]
    if "t5" in want:
        assert d["t5"] == want["t5"] and d["t3"] == want["t3"] and d["internal"] == want["internal"]
    if name == "coords":
        assert "t5" in want and len(want["internal"]) > 10 and min(want["internal"]) < 0      # the unsorted regions give negative gaps, as written


def test_outlier_data(emu_estimates, emu_lib):
    for nm in ("length_bias", "unanimous_5000", "many_unmapped", "low_coverage"):
        t = emu_estimates[nm]
        out = t.outlier_data(lib=emu_lib)
        assert BY_NAME[nm]["warnings"] == [[list(w) for w in t.get_warnings()]], (nm, t.get_warnings(), BY_NAME[nm]["warnings"])
        if nm in ("many_unmapped", "low_coverage"):
            assert out["lines"] is None and not out["warning"]
        else:
            assert out["lines"] == (t.get_mean() - 3 * t.get_sd(), t.get_mean() + 3 * t.get_sd()) and out["warning"] == (nm == "length_bias")
    t = emu_estimates["length_bias"]
    assert t.outlier_data(lib=emu_lib)["outliers"].tolist() == [5, 6] and len(t.get_warnings()) == 1      # the bins from 15000 bases on; the warning once


def test_the_constructor_loads_no_library_and_the_estimate_leaves_its_fields(table_paths, emu_lib, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(api, "load_library", refuse)
    t = CoverageTable(table_paths["unanimous_400"])
    assert t.get_mean() is None and t.is_low_coverage() is None and t.is_no_coverage() is None and list(t.get_warnings()) == [] and t.get_logn_mode() is None
    t.selected_coverage(), t.terminal_data()
    fields = ("names", "qlen", "n_mbase", "good_coords", "med_coords", "t1_cov", "qv", "div", "cov", "unmapped_frac_trimmed", "unmapped_frac_untrimmed",
              "unmapped_frac_med", "high_div_frac", "control_reads")
    before = {f: (getattr(t, f).copy() if isinstance(getattr(t, f), np.ndarray) else getattr(t, f)) for f in fields}
    with pytest.raises(AssertionError):
        t.est_coverage()                                            # (without a library given, the estimate asks for one)
    t.est_coverage(lib=emu_lib)
    for f in fields:
        now = getattr(t, f)
        assert (now.tobytes() == before[f].tobytes()) if isinstance(now, np.ndarray) else (now == before[f]), f


def write_table(path, covs):
    with open(path, "w") as f:
        for i, c in enumerate(covs):
            text = "0.0" if c == 0 else "%.3f" % c
            f.write("\t".join(["r%d" % i, "1000", "0" if c == 0 else "5000", "0" if c == 0 else "10-990", "0" if c == 0 else "10-990", text, "9.000", "0.100", text]) + "\n")
    return str(path)


def test_what_crashes_the_reference_is_a_value_error(tmp_path, emu_lib):
    for name, covs, word in (("one", [0] * 7 + [1.0, 2.0, 3.0], "one selected"), ("flat", [0] * 10 + [1.0] * 5 + [3.0] * 5, "no variance"),
                             ("negative", [-5, -4, -3, -2.5, -2, -1.5, -1, -0.5, 1, 2], "not positive")):
        t = CoverageTable(write_table(tmp_path / (name + ".txt"), covs))
        with pytest.raises(ValueError, match=word):
            t.est_coverage(lib=emu_lib)
    many = CoverageTable(write_table(tmp_path / "many.txt", [0.001 * (i + 1) for i in range(12000)]))
    with pytest.raises(ValueError, match="at most %d" % M.MAX_N):
        many.est_coverage(lib=emu_lib)
    with pytest.raises(ValueError, match="2 to %d" % M.MAX_N):
        many.bootstrap_main(4, lib=emu_lib)


def test_the_restated_argrelmax_is_scipys():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(2)
    for h in ([], [1.0], [1.0, 2.0], [1, 3, 2], [1, 3, 3, 2], [5, 1, 5], [0, 1, 0, 1, 0], [2, 2, 2], [math.nan, 1, 0, 2, math.nan, 3, 1], rng.random(200), rng.integers(0, 4, 300)):
        h = np.asarray(h, dtype=np.float64)
        assert CoverageTable.relative_maxima(h).tolist() == (signal.argrelmax(h)[0].tolist() if h.size else [])


def check_bootstrap(t, lib):
    a, b = t.bootstrap_main(nbs=24, seed=5, lib=lib), t.bootstrap_main(nbs=24, seed=5, lib=lib)
    assert a["mean"].tobytes() == b["mean"].tobytes() and a["sd"].tobytes() == b["sd"].tobytes() and a["mean_ci"] == b["mean_ci"]
    assert a["mean"].shape == (24,) and np.isfinite(a["mean"]).all() and np.isfinite(a["sd"]).all() and (a["sd"] > 0).all()
    assert a["mean_ci"][0] <= np.median(a["mean"]) <= a["mean_ci"][1] and a["mean_ci"] == tuple(np.percentile(a["mean"], [0.5, 99.5]))
    assert t.bootstrap_main(nbs=24, seed=6, lib=lib)["mean"].tobytes() != a["mean"].tobytes()
    n = t.selected.size

    class Identity(np.random.Generator):                            # a generator whose draw is every row once, in two orders
        def integers(self, low, high, size):
            assert (low, high, size) == (0, n, (2, n))
            return np.array([np.arange(n), np.arange(n)[::-1]])
    same = t.bootstrap_main(nbs=2, seed=Identity(np.random.PCG64(0)), lib=lib)
    assert same["mean"].tolist() == [t.get_mean()] * 2 and same["sd"].tolist() == [float(t.get_sd())] * 2      # the identity resample, in two orders
    idx = np.random.default_rng(5).integers(0, n, size=(24, n))
    for k in (0, 11, 23):                                           # the batch is the single calls
        one = M.gmm2(t.selected[idx[k]], lib=lib)
        assert one["mu"][M.main_component(one)] == a["mean"][k] and math.sqrt(one["var"][M.main_component(one)]) == a["sd"][k]


def test_emulated_bootstrap(emu_estimates, emu_lib):
    check_bootstrap(emu_estimates["unanimous_400"], emu_lib)


@pytest.mark.gpu
def test_gpu_estimates_and_bootstrap(table_paths, gpu_lib):
    got = estimates(table_paths, gpu_lib)
    for nm in NAMES:
        check_estimate(BY_NAME[nm], got[nm])
    check_bootstrap(got["unanimous_400"], gpu_lib)

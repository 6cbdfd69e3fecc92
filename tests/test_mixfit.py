"""The two mixture fits of the coverage estimate (k_mix_gmm2 / k_mix_lognorm of kernels_mixfit.hpp behind lqmix_gmm2 / lqmix_lognorm;
longqc_amd/mixfit.py) under the wave emulator and on the GPU, against tests/golden/mixfit_cases.json (written by
tests/golden/make_mixfit_golden.py with sklearn, the reference's lq_coverage.py and mixEM) and the numpy model tests/mixfit_model.py.

  1. one step: tol < 0 with max_iter 1 and 2 (one mixEM pass: max_iter 0) against the model, whose sums are math.fsum.  THE BOUND is first
     order in u = 2^-53 and weighted by the terms themselves, as tests/test_figdata_kde.py weighs its own: a sum of n non-negative terms
     added in any order carries its terms' relative error plus n u; per value, y = x pc - mu pc is off by u (a + |y|), a = (|x| + |mu|) pc
     (the cancellation), and from there each line of gmm_step_bound() and logn_pass() names the roundings it counts.  The model makes the
     same roundings but in its sums, so twice the figure bounds |kernel - model|.  The start (r is 0 or 1, no exp) is off by (n + 3) u in a
     mean; the first iteration sees that error times its own condition, measured on the model by differences.  The second iteration is
     compared with the model's step from the kernel's own first, so nothing is carried.  The data are positive (x > 1 for mixEM's pass,
     whose log-densities the test asserts negative): every sum but the bound's has terms of one sign.  WHAT IT CANNOT SEE: the figure is a
     worst case (every rounding at its limit, the start's error times a condition taken by differences, then doubled) and comes to 3e-12 ..
     1e-10 where the errors met are below 1e-15, so it catches a slip in a formula, a missing term or a wrong constant, which are off by
     1e-8 or more, but not a sum added in another order or a regrouping such as (r d) d against r (d d), which move a result by a few
     units of 2^-53.  The order of the sums is pinned by test 5 instead (the same bytes whatever the grid, the batch and the thread
     order), the grouping by the golden cases only as far as their tolerances reach;
  2. unanimous golden cases: n_iter is the reference's, every parameter within max(8 w, n_iter n 2^-53 |v|) of the seeds' range, w the
     recorded width over the seeds (the reference's own rounding noise);
  3. split cases: every parameter inside the seeds' [min, max] widened by n_iter n 2^-53 |v|, n_iter one of the recorded ones;
  4. log-normal from a fixed start: parameters within max(8 w_perm, n_iter n 2^-53 |v|) of mixEM's under 4 row orders, the exit kind
     equal, n_iter at most 501;
  5. determinism: byte-identical lqmix_fit under every thread order of the emulator, twice on the GPU, with LQMIX_TEST_MAX_BLOCKS=1, alone
     and as segment 0, middle and last of a batch of unequal segments, and with the rows permuted;
  6. shapes: n = 2, 3, 255, 256, 257, 65 (one past the block's 64 threads), LQ_MIX_MAX_N; two distinct values repeated; best splits at
     k = 1 and k = n - 1; equal squared errors at two splits (the smaller k wins);
  7. refusals (LQCOV_E_ARG): n < 2, equal values, n_fits = 0, NaN, LQ_MIX_MAX_N + 1 values; mixEM's NaN exit is reported, not raised."""
import json
import math
import os

import numpy as np
import pytest

from longqc_amd import api
from longqc_amd import mixfit as M
from tests import mixfit_model as MM
from tests import test_launch_caps as LC
from tests.conftest import GOLDEN

U = 2.0 ** -53
CASES = json.load(open(os.path.join(GOLDEN, "mixfit_cases.json")))
TABLES = {c["name"]: c for c in CASES["tables"]}
MAX_N = LC.header_define("LQ_MIX_MAX_N")


def selected_of(case):
    from longqc_amd.covtable import CoverageTable
    import gzip
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.txt")
        with open(p, "wb") as f:
            f.write(gzip.open(os.path.join(GOLDEN, case["file"])).read())
        return CoverageTable(p).selected_coverage()


_SELECTED = {}


def selected(name):
    if name not in _SELECTED:
        _SELECTED[name] = selected_of(TABLES[name])
    return _SELECTED[name]


def test_the_header_agrees_with_the_python_side():
    assert MAX_N == M.MAX_N == LC.header_define("LQ_MIX_TILE") * LC.header_define("LQ_MIX_MAX_TILES")
    assert LC.header_define("LQ_MIX_THREADS") == 64 and LC.header_define("LQ_MIX_TILE") == LC.header_define("LQ_FIG_TILE")
    kinds = [c["kind"] for c in CASES["tables"]]
    assert kinds.count("unanimous") >= 2 and kinds.count("split") >= 3 and "no_coverage" in kinds


# ---- 1. one step --------------------------------------------------------------------------------------------------------------------
def gmm_start(x, reg_covar):
    """the model's start (the M-step from the best split's one-hot responsibilities) -> (k, (w, mu, var), its relative error bound)"""
    n = x.size
    k = MM.best_split(x)
    r = np.array([np.arange(n) < k, np.arange(n) >= k], dtype=np.float64)
    nk, mu, var = MM._gmm_params(x, r, reg_covar)
    e = 0.0
    for j in (0, 1):
        d = np.abs(x - mu[j])[r[j] > 0]
        e_mu = (n + 3) * U
        e = max(e, e_mu, ((n + 5) * U * float((d * d).sum()) + 2 * abs(mu[j]) * e_mu * float(d.sum())) / (nk[j] * var[j]) + 3 * U)
    return k, (nk / n, mu, var), e


def gmm_step(x, p, reg_covar):
    """one E/M iteration of the model from p = (w, mu, var) -> (w, mu, var, bound)"""
    r, lse = MM.gmm_resp(x, *p)
    nk, mu, var = MM._gmm_params(x, r, reg_covar)
    return nk / (nk[0] + nk[1]), mu, var, MM.fsum(lse) / x.size


def gmm_step_bound(x, p, reg_covar):
    """the first-order bound of the docstring on one iteration from exact p -> (relative bound on w / mu / var, absolute on the bound)"""
    w, mu, var = p
    n, pc = x.size, 1.0 / np.sqrt(var)
    r, lse = MM.gmm_resp(x, w, mu, var)
    d = []
    for j in (0, 1):
        y = np.abs(x * pc[j] - mu[j] * pc[j])
        a = (np.abs(x) + abs(mu[j])) * pc[j]
        wl = np.abs(-0.5 * (MM.LOG_2PI + y * y) + math.log(pc[j]) + math.log(w[j]))
        d.append((y * (a + y) + y * y + 3 * (wl + 6)) * U)           # wl: y's error times |y|, the square's and the three additions' roundings
    d_lse = np.maximum(d[0], d[1]) + (6 + np.abs(lse)) * U           # lse: the larger wl's error, two exp, a log, two additions
    nk, mu2, var2 = MM._gmm_params(x, r, reg_covar)
    rel, e_nk = 0.0, []
    for j in (0, 1):
        g = d[j] + d_lse + (np.abs(np.log(np.maximum(r[j], 1e-320))) + 2) * U      # r = exp(wl - lse), relative
        e_nk.append(float((r[j] * (g + (n + 2) * U)).sum() / r[j].sum()) + U)
        e_mu = float((r[j] * x * (g + (n + 3) * U)).sum() / (r[j] * x).sum()) + e_nk[j] + U
        dd = np.abs(x - mu2[j])                                    # the new mean moves every difference: Cauchy-Schwarz on sum r |x - mu|
        e_var = (float((r[j] * dd * dd * (g + (n + 5) * U)).sum()) + 2 * abs(mu2[j]) * e_mu * float((r[j] * dd).sum())) / (nk[j] * var2[j]) + e_nk[j] + 2 * U
        rel = max(rel, e_mu, e_var)
    rel = max(rel, 2 * max(e_nk) + 2 * U)
    return rel, float((d_lse.sum() + (n + 2) * U * np.abs(lse).sum()) / n)


def gmm_step_condition(x, p, reg_covar, h=1e-7):
    """how much a relative error of the step's input shows in its output, first order: the largest sum over the six inputs of
    |relative change of an output| / h (the bound: absolute change), by one-sided differences of the model's step"""
    base = gmm_step(x, p, reg_covar)
    flat = np.concatenate(base[:3])
    rel, ab = np.zeros(6), 0.0
    for which in range(3):
        for j in (0, 1):
            q = [np.array(v, dtype=np.float64) for v in p]
            q[which][j] *= 1 + h
            if which == 0:
                q[0] = q[0] / q[0].sum()
            out = gmm_step(x, tuple(q), reg_covar)
            rel += np.abs(np.concatenate(out[:3]) - flat) / np.abs(flat) / h
            ab += abs(out[3] - base[3]) / h
    return float(rel.max()), ab


def assert_gmm_steps(x, iters, lib, reg_covar=1e-6):
    """iters 1: the kernel's first iteration against the model's, the start's error carried through the step's condition; iters 2: the
    kernel's second iteration against the model's step from the kernel's own first (the same bytes as its inner state: test 5)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    assert (x > 0).all()
    k, p, e_start = gmm_start(x, reg_covar)
    got = M.gmm2(x, tol=-1.0, max_iter=iters, reg_covar=reg_covar, lib=lib)
    assert got["n_iter"] == iters and got["exit"] == "max" and got["n"] == n
    if iters == 1:
        cond, cond_ll = gmm_step_condition(x, p, reg_covar)
        step, ll_abs = gmm_step_bound(x, p, reg_covar)
        rel, ll_abs = 2 * step + 2 * cond * e_start, 2 * ll_abs + 2 * cond_ll * e_start
    else:
        first = M.gmm2(x, tol=-1.0, max_iter=1, reg_covar=reg_covar, lib=lib)
        p = (first["w"], first["mu"], first["var"])
        step, ll_abs = gmm_step_bound(x, p, reg_covar)
        rel, ll_abs = 2 * step, 2 * ll_abs
    w, mu, var, ll = gmm_step(x, p, reg_covar)
    o = [1, 0] if mu[1] < mu[0] else [0, 1]
    want = {"w": w[o], "mu": mu[o], "var": var[o], "ll": ll, "split": k}
    assert rel < 1e-6, rel                                         # (a bound that says something: a slip in a formula is off by far more)
    for key in ("w", "mu", "var"):
        err = np.abs(got[key] - want[key]) / np.abs(want[key])
        print("n %d iters %d %s: error %.3g, bound %.3g" % (n, iters, key, float(err.max()), rel))
        assert (err <= rel).all(), (n, iters, key, got[key], want[key], rel)
    assert abs(got["ll"] - want["ll"]) <= ll_abs, (got["ll"], want["ll"], ll_abs)
    return got, want


def mixture(rng, n, main=30.0, sd=3.0, bg=0.3):
    nb = max(1, int(n * bg))
    return np.round(np.concatenate([rng.uniform(0.5, 3 * main, nb), np.abs(rng.normal(main, sd, n - nb)) + 0.5]), 3)


def check_one_gmm_step(lib):
    rng = np.random.default_rng(3)
    for n in (300, 1000):
        x = mixture(rng, n)
        for iters in (1, 2):
            assert_gmm_steps(x, iters, lib)
    assert_gmm_steps(mixture(rng, 500), 1, lib, reg_covar=0.5)       # (reg_covar where it shows)


def logn_pass(x, start):
    """one mixEM pass by the model from the exact start -> (fit, relative bound on w / mu / sigma, absolute bound on ll)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    lx, n = np.log(x), x.size
    assert (x > 1).all()
    fit = MM.lognorm_norm(x, start, max_iter=0)
    mu, sg, data = (start[0], start[2]), (start[1], start[3]), (x, lx)
    r0, r1, e = MM.logn_resp(x, lx, [1.0, 1.0], mu, sg)
    r, l, d = (r0, r1), [], []
    for j in (0, 1):
        u1 = np.abs(data[j] - mu[j])
        q = u1 * u1 / (2 * sg[j] ** 2)
        lj = -q - math.log(sg[j]) - MM.HALF_LOG_2PI - (lx if j else 0.0)
        dj = 6 * U * q + 3 * U * (np.abs(lj) + abs(math.log(sg[j])) + 1)
        if j:
            dj = dj + (2 * u1 * np.abs(lx) / (2 * sg[j] ** 2) + 4 * np.abs(lx)) * U        # log x is rounded once
        l.append(lj)
        d.append(dj)
    assert (l[0] < 0).all() and (l[1] < 0).all()                   # the terms of ll have one sign
    rel, ll_abs = 0.0, (n + 1) * U * abs(fit["ll"])
    for j in (0, 1):
        g = d[j] + np.maximum(d[0], d[1]) + 8 * U
        ll_abs += float((r[j] * np.abs(l[j]) * (g + 2 * U) + r[j] * d[j]).sum())
        e_ws = float((r[j] * (g + (n + 1) * U)).sum() / r[j].sum())
        e_mu = float((r[j] * data[j] * (g + (n + 4) * U)).sum() / (r[j] * data[j]).sum()) + e_ws + U
        dd = np.abs(data[j] - fit["mu"][j])
        s2 = float((r[j] * dd * dd).sum())
        shift = abs(fit["mu"][j]) * e_mu + (float(np.abs(lx).max()) * U if j else 0.0)
        e_sg = 0.5 * ((float((r[j] * dd * dd * (g + (n + 5) * U)).sum()) + 2 * shift * float((r[j] * dd).sum())) / s2 + e_ws + 2 * U) + U
        rel = max(rel, e_ws + U, e_mu, e_sg)
    return fit, 2 * rel, 2 * ll_abs


def assert_logn_pass(x, start, lib):
    want, rel, ll_abs = logn_pass(x, start)
    got = M.lognorm_norm(x, start, max_iter=0, lib=lib)
    assert got["n_iter"] == 1 and got["exit"] == "max" and rel < 1e-6
    for key in ("w", "mu", "sigma"):
        err = np.abs(got[key] - want[key]) / np.abs(want[key])
        print("n %d %s: error / bound %.3g" % (len(x), key, float((err / rel).max())))
        assert (err <= rel).all(), (len(x), key, got[key], want[key], rel)
    assert abs(got["ll"] - want["ll"]) <= ll_abs


def check_one_logn_pass(lib):
    rng = np.random.default_rng(4)
    for n in (200, 700):
        x = np.round(np.concatenate([rng.uniform(1.5, 40, n // 3), np.exp(rng.normal(2.5, 0.3, n - n // 3)) + 1.0]), 3)
        assert_logn_pass(x, (15.0, 9.0, 2.2, 1.0), lib)


# ---- 2, 3. the golden tables ----------------------------------------------------------------------------------------------------------
def seeds_range(case, key):
    lo, hi = case["gmm_range"][key]
    return np.array(lo), np.array(hi)


def assert_in_seeds_range(case, fit, n):
    """the tolerances of 2 (unanimous) and 3 (split) on w, mu, var and n_iter"""
    assert fit["n_iter"] in case["n_iters"], (case["name"], fit["n_iter"], case["n_iters"])
    for key in ("w", "mu", "var"):
        lo, hi = seeds_range(case, key)
        rounding = fit["n_iter"] * n * U * np.abs(fit[key])
        slack = np.maximum(8 * (hi - lo), rounding) if case["kind"] == "unanimous" else rounding
        out = np.maximum(lo - fit[key], fit[key] - hi)
        print("%s %s: outside the seeds' range by %s, allowed %s" % (case["name"], key, out, slack))
        assert (out <= slack).all(), (case["name"], key, fit[key], lo, hi, slack)


def check_golden_tables(lib):
    names = [c["name"] for c in CASES["tables"] if c["kind"] != "no_coverage"]
    fits = M.gmm2_many([selected(nm) for nm in names], lib=lib)    # one launch
    for nm, fit in zip(names, fits):
        assert fit["n"] == TABLES[nm]["selected"] and fit["exit"] == "tol"
        assert_in_seeds_range(TABLES[nm], fit, fit["n"])


# ---- 4. log-normal from a fixed start -------------------------------------------------------------------------------------------------
def check_golden_lognorm(lib):
    for c in CASES["lognorm"]:
        x = np.cumsum(c["x_thou_steps"]) / 1000
        got = M.lognorm_norm(x, c["start"], lib=lib)
        print("%s: n_iter %d (the model's %d), exit %s" % (c["name"], got["n_iter"], c["n_iter"], got["exit"]))
        assert got["exit"] == c["exit"] and 1 <= got["n_iter"] <= 501 and got["n"] == x.size
        if c["exit"] == "nan":
            assert math.isnan(got["ll"]) and np.isnan(got["mu"]).all()
            continue
        for key in ("w", "mu", "sigma"):
            v = np.array([r[key] for r in c["runs"]])
            tol = np.maximum(8 * (v.max(axis=0) - v.min(axis=0)), got["n_iter"] * x.size * U * np.abs(got[key]))
            out = np.maximum(v.min(axis=0) - got[key], got[key] - v.max(axis=0))
            assert (out <= tol).all(), (c["name"], key, got[key], v, tol)


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------
def segments():
    rng = np.random.default_rng(8)
    main = selected("split_b")
    return main, [mixture(rng, 37), mixture(rng, 700, 12.0, 2.0), mixture(rng, 2), mixture(rng, 1300, 50.0, 9.0)]


def fits_every_way(lib):
    """the same segment alone, first, in the middle and last in a batch, and permuted -> the records' bytes (all must be one value), and
    the log-normal fit of it the same ways"""
    main, others = segments()
    perm = main[np.random.default_rng(9).permutation(main.size)]
    g = [M.gmm2_raw([main], lib=lib)[0], M.gmm2_raw([main] + others, lib=lib)[0], M.gmm2_raw(others[:2] + [main] + others[2:], lib=lib)[2],
         M.gmm2_raw(others + [main], lib=lib)[4], M.gmm2_raw([perm], lib=lib)[0]]
    start = (4.0, 5.0, 2.5, 1.0)
    inits = [start] * 5
    l = [M.lognorm_norm_raw([main], [start], lib=lib)[0], M.lognorm_norm_raw([main] + others, inits, lib=lib)[0],
         M.lognorm_norm_raw(others[:2] + [main] + others[2:], inits, lib=lib)[2], M.lognorm_norm_raw(others + [main], inits, lib=lib)[4],
         M.lognorm_norm_raw([perm], [start], lib=lib)[0]]
    return [r.tobytes() for r in g], [r.tobytes() for r in l]


def assert_one_value(seen):
    g = {b for run in seen for b in run[0]}
    l = {b for run in seen for b in run[1]}
    assert len(g) == 1 and len(l) == 1, (len(g), len(l))
    fit = np.frombuffer(next(iter(g)), dtype=M.FIT)[0]
    assert fit["n_iter"] >= 2 and np.isfinite(fit["mu"]).all()


# ---- 6. shapes ------------------------------------------------------------------------------------------------------------------------
def check_shapes(lib):
    rng = np.random.default_rng(6)
    for n in (2, 3, 255, 256, 257, 65):
        if n <= 3:                                                  # (clusters of one value: reg_covar is all their variance, 1.0 keeps the step well conditioned)
            x = np.array([3.25, 7.5, 4.0][:n])
            assert_gmm_steps(x, 1, lib, reg_covar=1.0)
            assert_gmm_steps(x, 2, lib, reg_covar=1.0)
            continue
        x = mixture(rng, n)
        assert_gmm_steps(x, 1, lib)
        assert_gmm_steps(x, 2, lib)
    two = np.array([4.0] * 130 + [9.5] * 131)                     # two distinct values repeated
    got, want = assert_gmm_steps(two, 1, lib)
    assert want["split"] == 130 and abs(got["mu"][0] - 4.0) < 1e-9 and abs(got["mu"][1] - 9.5) < 1e-9
    first = np.concatenate([[0.5], 40 + np.arange(50) * 0.125])   # the best split is k = 1
    last = np.concatenate([10 + np.arange(50) * 0.125, [90.0]])   # ... and k = n - 1
    assert MM.best_split(first) == 1 and MM.best_split(last) == 50
    assert_gmm_steps(first, 1, lib, reg_covar=0.01)
    assert_gmm_steps(last, 1, lib, reg_covar=0.01)
    tie = np.array([1.0, 2.0, 3.0])                                # {1} + {2, 3} and {1, 2} + {3}: the same squared error, k = 1 wins
    got, want = assert_gmm_steps(tie, 1, lib, reg_covar=0.01)
    assert want["split"] == 1
    other = MM.gmm2(tie, split=2, tol=-1.0, max_iter=1, reg_covar=0.01)
    assert abs(got["mu"][0] - other["mu"][0]) > 1e-3 * other["mu"][0], (got, other)


def check_full_size(lib):
    rng = np.random.default_rng(7)
    x = mixture(rng, MAX_N, 25.0, 2.5, 0.2)
    assert_gmm_steps(x, 1, lib)
    assert_gmm_steps(x, 2, lib)
    assert_logn_pass(x + 1.0, (30.0, 20.0, 3.2, 1.0), lib)
    fit = M.gmm2(x, lib=lib)                                        # the whole loop at full size ends by its own rule
    assert fit["exit"] == "tol" and 2 <= fit["n_iter"] < 100 and abs(fit["mu"][M.main_component(fit)] - 25.0) < 0.5
    with pytest.raises(api.LqcovError) as e:
        M.gmm2(np.concatenate([x, [1.0]]), lib=lib)
    assert e.value.code == -1


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    good = np.array([1.0, 2.0, 4.0, 8.0])
    for bad in ([good[:1]], [good, np.zeros(0)], [np.full(7, 2.5)], [], [np.array([1.0, math.nan, 3.0])], [np.array([1.0, math.inf])]):
        for call in (lambda a: M.gmm2_many(a, lib=lib), lambda a: M.lognorm_norm_many(a, [(1.0, 1.0, 1.0, 1.0)] * len(a), lib=lib)):
            with pytest.raises(api.LqcovError) as e:
                call(bad)
            assert e.value.code == -1, bad                          # LQCOV_E_ARG
    for kw in ({"max_iter": 0}, {"reg_covar": -1.0}, {"tol": math.nan}):
        with pytest.raises(api.LqcovError) as e:
            M.gmm2(good, lib=lib, **kw)
        assert e.value.code == -1
    for x, init, kw in ((np.array([0.0, 1.0, 2.0]), (1, 1, 1, 1), {}), (good, (1, 0.0, 1, 1), {}), (good, (1, 1, math.nan, 1), {}), (good, (1, 1, 1, 1), {"tol_iters": 0}),
                        (good, (1, 1, 1, 1), {"tol_iters": 65})):
        with pytest.raises(api.LqcovError) as e:
            M.lognorm_norm(x, init, lib=lib, **kw)
        assert e.value.code == -1
    nan = M.lognorm_norm(np.array([1.0, 1.5, 2.0, 2.5, 1e6]), (2.0, 0.5, 0.5, 0.1), lib=lib)      # both densities of 1e6 underflow: reported
    assert nan["exit"] == "nan" and nan["n_iter"] == 1 and math.isnan(nan["ll"])
    assert M.main_component({"w": [0.3, 0.7], "var": [1.0, 9.0]}) == 0 and M.main_component({"w": [0.3, 0.7], "var": [9.0, 1.0]}) == 1


# ---- under the emulator ---------------------------------------------------------------------------------------------------------------
def test_emulated_one_step(emu_lib):
    check_one_gmm_step(emu_lib)
    check_one_logn_pass(emu_lib)


def test_emulated_golden_tables(emu_lib):
    check_golden_tables(emu_lib)


def test_emulated_golden_lognorm(emu_lib):
    check_golden_lognorm(emu_lib)


def test_emulated_fits_are_the_same_bytes_every_way(emu_lib, monkeypatch):
    monkeypatch.delenv("LQMIX_TEST_MAX_BLOCKS", raising=False)
    seen = []
    for order in LC.ORDERS:
        LC.set_order(monkeypatch, order)
        seen.append(fits_every_way(emu_lib))
    monkeypatch.setenv("LQMIX_TEST_MAX_BLOCKS", "1")
    seen.append(fits_every_way(emu_lib))
    assert_one_value(seen)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_shapes(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_shapes(emu_lib)


def test_emulated_full_size(emu_lib):
    check_full_size(emu_lib)


def test_emulated_refusals(emu_lib):
    check_refusals(emu_lib)


def test_the_golden_fit_is_sklearns():
    """where sklearn imports: one unanimous case refitted is the file's -- the golden file is pinned to the library"""
    mixture_mod = pytest.importorskip("sklearn.mixture")
    case = TABLES["unanimous_400"]
    np.random.seed(0)
    m = mixture_mod.GaussianMixture(n_components=2).fit(selected("unanimous_400").reshape(-1, 1))
    o = np.argsort(m.means_.ravel())
    assert m.n_iter_ in case["n_iters"]
    assert np.allclose(m.means_.ravel()[o], case["seed_fits"]["0"]["gmm"]["mu"], rtol=1e-9, atol=0)
    assert np.allclose(m.covariances_.ravel()[o], case["seed_fits"]["0"]["gmm"]["var"], rtol=1e-9, atol=0)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_one_step(gpu_lib):
    check_one_gmm_step(gpu_lib)
    check_one_logn_pass(gpu_lib)


@pytest.mark.gpu
def test_gpu_golden_tables(gpu_lib):
    check_golden_tables(gpu_lib)


@pytest.mark.gpu
def test_gpu_golden_lognorm(gpu_lib):
    check_golden_lognorm(gpu_lib)


@pytest.mark.gpu
def test_gpu_fits_are_the_same_bytes_every_way(gpu_lib, monkeypatch):
    monkeypatch.delenv("LQMIX_TEST_MAX_BLOCKS", raising=False)
    seen = [fits_every_way(gpu_lib), fits_every_way(gpu_lib)]
    monkeypatch.setenv("LQMIX_TEST_MAX_BLOCKS", "1")
    seen.append(fits_every_way(gpu_lib))
    assert_one_value(seen)


@pytest.mark.gpu
def test_gpu_shapes(gpu_lib):
    check_shapes(gpu_lib)


@pytest.mark.gpu
def test_gpu_full_size(gpu_lib):
    check_full_size(gpu_lib)


@pytest.mark.gpu
def test_gpu_refusals(gpu_lib):
    check_refusals(gpu_lib)

#!/usr/bin/env python3
"""Writes tests/golden/figdata_cases.json: the inputs and the expected numbers of the figure-data tests (tests/test_figdata_*.py).
Run where scipy is installed: python tests/golden/make_figdata_golden.py.  Doubles are stored as float.hex() strings, float32 inputs as
their bit patterns (8 hex digits each, concatenated): the file carries its inputs and does not lean on a random stream staying the same.

Per KDE case: the fractions, n, the bandwidth h that scipy.stats.gaussian_kde(x) uses (its Cholesky factor), and for each of the 50
points np.linspace(0, 1, 50):
  exact   the density sum_i exp(-u^2 / 2) / n / (h sqrt(2 pi)), u = (p - d_i) / h, from the doubles' exact values with Python's decimal
          at 60 digits, rounded to the nearest double (0.0 where it lies below 2^-1075; `underflow` lists those points)
  scipy   gaussian_kde(x)(points)
  tol     the first-order bound of a double evaluation that takes the difference first, relative to the exact value:
          sum_i term_i (3 t_i + 300) 2^-53 / sum_i term_i, t_i = u^2 / 2 -- 3 t_i for the roundings of the difference, the quotient and
          the square that exp carries into its result, 300 for one ulp of exp, at most 256 sequential additions and the tree.
Per length case: the lengths and scipy.stats.gamma.fit(lengths, floc=0) as [a, scale], or the name of the exception it raises."""
import json
import math
import os
from decimal import Decimal, getcontext

import numpy as np
from scipy.stats import gamma, gaussian_kde

HERE = os.path.dirname(os.path.abspath(__file__))
getcontext().prec = 60
XS = np.linspace(0, 1.0, 50)
HALF_DENORMAL = Decimal(2) ** -1075


def exact_curve(x32, h):
    """-> (exact densities as Decimal, tol as float) at XS"""
    d = [Decimal(float(v)) for v in x32]
    H = Decimal(h)
    norm = len(d) * H * (2 * Decimal("3.14159265358979323846264338327950288419716939937510582097494")).sqrt()
    dens, tol = [], []
    for p in XS:
        P = Decimal(float(p))
        tot = w = Decimal(0)
        for v in d:
            u = (P - v) / H
            t = u * u / 2
            term = (-t).exp()
            tot += term
            w += term * (3 * t + 300)
        dens.append(tot / norm)
        tol.append(float(w / tot * Decimal(2) ** -53))
    return dens, tol


def kde_case(name, x32):
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    k = gaussian_kde(x32)
    h = float(k.cho_cov[0, 0])
    assert math.isclose(h, math.sqrt(float(np.cov(x32.astype(np.float64), ddof=1))) * k.neff ** (-1. / 5), rel_tol=2.0 ** -50)
    dens, tol = exact_curve(x32, h)
    return {"name": name, "n": int(x32.shape[0]), "x_f32_hex": x32.view(np.uint32).astype(">u4").tobytes().hex(), "h": h.hex(),
            "exact": [float(v).hex() for v in dens], "underflow": [j for j, v in enumerate(dens) if v < HALF_DENORMAL],
            "scipy": [float(v).hex() for v in k(XS)], "tol": [float(t).hex() for t in tol]}, dens


def gc_cloud():
    """n = 3000 fractions k / 150-like around 0.41, sd about 0.01: h is about 0.002, so the figure's end points underflow.  The seed is
    the first whose exact curve has points that are 0 in double, points in (1e-300, 1e-200) and points above 1e-6 of the peak"""
    for seed in range(100):
        rng = np.random.default_rng(1000 + seed)
        x = (0.41 + 0.01 * rng.standard_normal(3000)).astype(np.float32)
        case, dens = kde_case("gc_cloud", x)
        peak = max(dens)
        if case["underflow"] and any(Decimal("1e-300") < v < Decimal("1e-200") for v in dens) and sum(v > peak / 10 ** 6 for v in dens) >= 3:
            case["seed"] = 1000 + seed
            return case
    raise SystemExit("no seed gives the three regimes")


def length_case(name, lens):
    lens = np.asarray(lens, dtype=np.uint32)
    out = {"name": name, "lengths": lens.tolist()}
    try:
        a, loc, scale = gamma.fit(lens, floc=0)
        assert loc == 0
        out["gamma_fit"] = [float(a).hex(), float(scale).hex()]
    except Exception as e:                                          # (n = 1 and all equal: brentq is handed s = 0)
        out["gamma_fit_raises"] = [c.__name__ for c in type(e).__mro__]
    return out


def main():
    rng = np.random.default_rng(7)
    kde = [gc_cloud()]
    kde.append(kde_case("two_values", np.array([0.25, 0.5], dtype=np.float32))[0])
    kde.append(kde_case("one_past_a_tile", rng.beta(20, 30, 257).astype(np.float32))[0])
    kde.append(kde_case("one_past_two_tiles", (np.round(150 * rng.beta(8, 12, 513)) / 150).astype(np.float32))[0])
    kde.append(kde_case("two_clusters", np.concatenate([0.2 + 0.004 * rng.standard_normal(300), 0.7 + 0.02 * rng.standard_normal(500)]).astype(np.float32))[0])
    lens = [length_case("gamma_like", np.maximum(1, rng.gamma(1.3, 8000.0, 5000)).astype(np.uint32)),
            length_case("one_read", [12345]),
            length_case("all_equal", [1500] * 40)]
    out = {"points": [float(p).hex() for p in XS], "kde": kde, "lengths": lens}
    path = os.path.join(HERE, "figdata_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    for c in kde:
        e = [float.fromhex(v) for v in c["exact"]]
        print(c["name"], c["n"], "h", float.fromhex(c["h"]), "underflow", len(c["underflow"]), "min>0", min([v for v in e if v > 0] or [0]), "peak", max(e),
              "max tol", max(float.fromhex(t) for t in c["tol"]))
    for c in lens:
        print(c["name"], c.get("gamma_fit"), c.get("gamma_fit_raises"))


if __name__ == "__main__":
    main()

"""A plain numpy model of the two mixture fits of longqc_amd/csrc/kernels_mixfit.hpp, for tests/test_mixfit.py and
tests/golden/make_mixfit_golden.py: the same formulas in the same order of operations, each term in double with numpy, every sum over the
data by math.fsum (exact, rounded once).  The kernels differ from it in the order of their sums (tiles of 256 in index order, a pairwise
tree) and in exp / log."""
import math

import numpy as np

LOG_2PI = float(np.log(2 * np.pi))
HALF_LOG_2PI = float(0.5 * np.log(2 * np.pi))
TEN_EPS = float(10 * np.finfo(np.float64).eps)


def fsum(a):
    return math.fsum(a.tolist())


def best_split(s):
    """the smallest k in [1, n - 1] at the minimum squared error of {s[:k]} + {s[k:]}, s ascending: running sums in sequential double"""
    s = [float(v) for v in s]
    n = len(s)
    t1 = t2 = 0.0
    for v in s:
        t1 += v
        t2 += v * v
    a1 = a2 = 0.0
    best, best_k = math.inf, 1
    for k in range(1, n):
        a1 += s[k - 1]
        a2 += s[k - 1] * s[k - 1]
        b1, b2 = t1 - a1, t2 - a2
        sse = (a2 - a1 * a1 / k) + (b2 - b1 * b1 / (n - k))
        if sse < best:
            best, best_k = sse, k
    return best_k


def _gmm_params(x, r, reg_covar, total=fsum):
    """sklearn's _estimate_gaussian_parameters for 1-D data -> (nk, mu, var)"""
    nk = np.array([total(r[0]) + TEN_EPS, total(r[1]) + TEN_EPS])
    mu = np.array([total(r[0] * x) / nk[0], total(r[1] * x) / nk[1]])
    var = np.array([total((r[k] * (x - mu[k])) * (x - mu[k])) / nk[k] + reg_covar for k in (0, 1)])
    return nk, mu, var


def gmm_resp(x, w, mu, var):
    """the E-step -> (r, per-value normalised log-probability)"""
    pc = 1.0 / np.sqrt(var)
    wl = []
    for k in (0, 1):
        y = x * pc[k] - mu[k] * pc[k]
        wl.append(((-0.5 * (LOG_2PI + y * y)) + math.log(pc[k])) + math.log(w[k]))
    m = np.maximum(wl[0], wl[1])
    lse = m + np.log(np.exp(wl[0] - m) + np.exp(wl[1] - m))
    return np.array([np.exp(wl[0] - lse), np.exp(wl[1] - lse)]), lse


def gmm2(x, split=None, tol=1e-3, max_iter=100, reg_covar=1e-6, total=fsum):
    """-> dict like mixfit.gmm2's; split: the start (default best_split of the sorted values)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    k = best_split(x) if split is None else split
    r = np.array([np.arange(n) < k, np.arange(n) >= k], dtype=np.float64)
    nk, mu, var = _gmm_params(x, r, reg_covar, total)
    w = nk / n
    bound, it, exit = -math.inf, 0, "max"
    while it < max_iter:
        it += 1
        prev = bound
        r, lse = gmm_resp(x, w, mu, var)
        bound = total(lse) / n
        nk, mu, var = _gmm_params(x, r, reg_covar, total)
        w = nk / (nk[0] + nk[1])
        if abs(bound - prev) < tol:
            exit = "tol"
            break
    o = [1, 0] if mu[1] < mu[0] else [0, 1]
    return {"w": w[o], "mu": mu[o], "var": var[o], "ll": bound, "n_iter": it, "exit": exit, "n": n, "split": k}


def logn_resp(x, lx, w, mu, sg):
    l0 = -((x - mu[0]) * (x - mu[0])) / (2.0 * (sg[0] * sg[0])) - math.log(sg[0]) - HALF_LOG_2PI
    l1 = -((lx - mu[1]) * (lx - mu[1])) / (2.0 * (sg[1] * sg[1])) - math.log(sg[1]) - HALF_LOG_2PI - lx
    with np.errstate(invalid="ignore", divide="ignore"):
        p0, p1 = w[0] * np.exp(l0), w[1] * np.exp(l1)
        tot = p0 + p1
        r0, r1 = p0 / tot, p1 / tot
        return r0, r1, r0 * l0 + r1 * l1


def lognorm_norm(x, init, tol=1e-15, tol_iters=10, max_iter=500, total=fsum):
    """mixem.em's loop -> dict like mixfit.lognorm_norm's"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    lx, n = np.log(x), x.size
    w, mu, sg = [1.0, 1.0], [float(init[0]), float(init[2])], [float(init[1]), float(init[3])]
    last = [0.0] * tol_iters
    it = 0
    while True:
        r0, r1, e = logn_resp(x, lx, w, mu, sg)
        ll = total(e) if np.isfinite(e).all() else math.nan
        s0, s1 = (total(r0), total(r1)) if ll == ll else (math.nan, math.nan)
        if ll == ll:
            mu = [total(r0 * x) / s0, total(r1 * lx) / s1]
            sg = [math.sqrt(total(r0 * ((x - mu[0]) * (x - mu[0]))) / s0), math.sqrt(total(r1 * ((lx - mu[1]) * (lx - mu[1]))) / s1)]
            w = [s0 / n, s1 / n]
        else:
            mu, sg, w = [math.nan] * 2, [math.nan] * 2, [math.nan] * 2
        if ll != ll:
            exit = "nan"
            break
        if it >= tol_iters and (last[-1] - ll) / last[-1] <= tol:
            exit = "tol"
            break
        if it >= max_iter:
            exit = "max"
            break
        last = [ll] + last[:-1]
        it += 1
    return {"w": np.array(w), "mu": np.array(mu), "sigma": np.array(sg), "ll": ll, "n_iter": it + 1, "exit": exit, "n": n}

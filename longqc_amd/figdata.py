"""The numbers behind LongQC's two distribution figures, over every read of a run, without scipy and without a host pass over the
arrays: what plot_unmasked_gc_frac computes before it draws (lq_gcfrac.py:49-85: two np.histogram, two scipy.stats.gaussian_kde
curves) and what estimate_gamma_dist_scipy / plot_length_dist need (lq_gamma.py:47-59, longQC.py:487-488,500: the length histogram
and gamma.fit(lengths, floc=0)).  The passes over the arrays run on the device (kernels_figdata.hpp) behind the four array-level
calls lqfig_range / lqfig_hist / lqfig_kde / lqfig_logsum of include/lqcov.h; what is left for the host works on a few numbers: the
bin edges (np.arange itself), the densities (numpy's own expression), the bandwidth, and the root of the gamma fit's equation.
Nothing is drawn: the caller plots the returned arrays.  No CPU fallback: without liblqcov.so or a HIP device the calls raise.

The two floating-point sums (kde_sums, log_sums) are added in an order fixed by the array's length alone: the same
input gives the same bytes on every call."""
import ctypes as C
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

from . import api

F32, U32 = 0, 1                                                    # LQFIG_F32 / LQFIG_U32


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqfig_bound", False):
        tail = [C.c_char_p, C.c_size_t]
        lib.lqfig_range.restype = lib.lqfig_hist.restype = lib.lqfig_kde.restype = lib.lqfig_logsum.restype = C.c_int
        lib.lqfig_range.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p] + tail
        lib.lqfig_hist.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p] + tail
        lib.lqfig_kde.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p] + tail
        lib.lqfig_logsum.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p] + tail
        lib._lqfig_bound = True
    return lib


def _box_lib(lib=None):
    """lqfig_boxstats bound on its own: a library that holds this call alone, or the four above alone, serves its callers"""
    lib = lib or api.load_library()
    if not getattr(lib, "_lqbox_bound", False):
        lib.lqfig_boxstats.restype = C.c_int
        lib.lqfig_boxstats.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_char_p, C.c_size_t]
        lib._lqbox_bound = True
    return lib


MISSING = -2 ** 31                                                 # LQFIG_MISSING: a "-nan" among the thousandths
# lqfig_box of include/lqcov.h
BOX = np.dtype([("group", np.uint32), ("reserved", np.uint32), ("first", np.uint64), ("n_all", np.uint64), ("n", np.uint64),
                ("mid_lo", np.int32), ("mid_hi", np.int32), ("q1", np.float64), ("med", np.float64), ("q3", np.float64),
                ("whislo", np.float64), ("whishi", np.float64), ("n_low", np.uint64), ("n_high", np.uint64)])
assert BOX.itemsize == 96


def _values(x, want=None):
    """x as a contiguous 1-D float32 or uint32 array (an array('f') is read in place) -> (array, LQFIG_* code)"""
    a = np.frombuffer(x, dtype=np.float32) if not isinstance(x, np.ndarray) and getattr(x, "typecode", None) == "f" and len(x) else np.asarray(x)
    if a.size == 0 and a.dtype not in (np.float32, np.uint32):
        a = a.astype(np.uint32 if want == U32 else np.float32)
    if a.ndim != 1 or a.dtype not in (np.float32, np.uint32) or (want is not None and a.dtype != (np.float32, np.uint32)[want]):
        raise TypeError("a 1-D array of %s is needed, not %s%s" % ("float32 or uint32" if want is None else ("float32", "uint32")[want], a.dtype, list(a.shape)))
    return np.ascontiguousarray(a), (F32 if a.dtype == np.float32 else U32)


def _check(rc, err):
    if rc != 0:
        raise api.LqcovError(rc, err.value.decode())


def _ptr(a):
    return a.ctypes.data if a.size else None


def value_range(x, device: int = 0, lib=None):
    """(min, max) of a float32 or uint32 array, of its own type (NaN left out); an empty array raises ValueError as min() does"""
    a, code = _values(x)
    if a.size == 0:
        raise ValueError("min() arg is an empty sequence")
    out = np.zeros(2, dtype=a.dtype)
    err = C.create_string_buffer(512)
    _check(_lib(lib).lqfig_range(device, code, _ptr(a), a.size, out.ctypes.data, out.ctypes.data + 4, err, 512), err)
    return out[0], out[1]


def hist(x, edges, device: int = 0, lib=None) -> np.ndarray:
    """np.histogram(x, bins=edges)[0] for an explicit edge array (int64 counts): edges[k] <= v < edges[k+1], the last bin closed on
    the right, values outside the edges and NaN counted nowhere.  Fewer than two edges: no bins"""
    a, code = _values(x)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    if e.ndim != 1:
        raise ValueError("edges must be 1-D")
    counts = np.zeros(max(e.size - 1, 0), dtype=np.uint64)
    err = C.create_string_buffer(512)
    _check(_lib(lib).lqfig_hist(device, code, _ptr(a), a.size, _ptr(e), e.size, _ptr(counts), err, 512), err)
    return counts.astype(np.int64)


def kde_sums(x, points, h: float, device: int = 0, lib=None) -> np.ndarray:
    """S[j] = sum_i exp(-0.5 u u), u = (points[j] - x[i]) / h in double, for float32 data: a Gaussian KDE before its normalisation"""
    a, _ = _values(x, F32)
    p = np.ascontiguousarray(points, dtype=np.float64).ravel()
    out = np.zeros(max(p.size, 1), dtype=np.float64)
    err = C.create_string_buffer(512)
    _check(_lib(lib).lqfig_kde(device, _ptr(a), a.size, _ptr(p), p.size, float(h), out.ctypes.data, err, 512), err)
    return out[:p.size]


def log_sums(x, device: int = 0, lib=None):
    """(sum of x as int, sum of log(x) over the non-zero values as float, the number of zeros) of a uint32 array"""
    a, _ = _values(x, U32)
    s, z, sl = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
    err = C.create_string_buffer(512)
    _check(_lib(lib).lqfig_logsum(device, _ptr(a), a.size, C.byref(s), C.byref(sl), C.byref(z), err, 512), err)
    return int(s.value), float(sl.value), int(z.value)


def scott_bandwidth(x) -> float:
    """the standard deviation of the Gaussian that scipy.stats.gaussian_kde(x) places on every value of a 1-D dataset (default
    bw_method, Scott's factor): sqrt(np.cov(x as float64, ddof=1)) * neff ** (-1/5), neff = 1 / sum((ones(n) / n) ** 2), through the
    operations scipy makes (its np.cov call carries the weights ones(n) / n; the Cholesky factor of the 1 x 1 data covariance is its
    square root, and the factor multiplies that).  One numpy pass on the host.  ValueError for fewer than two values and for zero variance"""
    d = np.atleast_2d(np.asarray(x))
    n = d.shape[1]
    if d.shape[0] != 1 or n < 2:
        raise ValueError("`dataset` input should have multiple elements.")
    w = np.ones(n) / n
    neff = 1 / np.sum(w ** 2)
    var = float(np.atleast_2d(np.cov(d, rowvar=1, bias=False, aweights=w))[0, 0])
    if not var > 0 or not math.isfinite(var):
        raise ValueError("the dataset has no variance: its covariance matrix is not positive definite")
    return float(math.sqrt(var) * np.power(neff, -1. / 5))


def gaussian_kde_curve(x, points, device: int = 0, lib=None, return_bandwidth: bool = False):
    """scipy.stats.gaussian_kde(x)(points) for a 1-D float32 dataset: kde_sums(x, points, h) / n / (h sqrt(2 pi)), h =
    scott_bandwidth(x).  ValueError where scipy raises ValueError or LinAlgError (fewer than two values, zero variance)"""
    a, _ = _values(x, F32)
    h = scott_bandwidth(a)
    curve = kde_sums(a, points, h, device, lib) / a.size / (h * math.sqrt(2 * math.pi))
    return (curve, h) if return_bandwidth else curve


def density_hist(x, start, stop, step, device: int = 0, lib=None, hist_fn=None):
    """-> (edges, counts, density): edges = np.arange(start, stop, step) whatever it yields, counts from hist, density = counts /
    np.diff(edges) / counts.sum(), numpy's expression and order: (density, edges) is np.histogram(x, bins=edges, density=True).
    hist_fn(edges) -> counts: for an array that lies on the device already (x is not looked at)"""
    edges = np.arange(start, stop, step)
    counts = hist(x, edges, device, lib) if hist_fn is None else hist_fn(edges)
    db = np.array(np.diff(edges), float)
    return edges, counts, counts / db / counts.sum()


# ---- box-plot statistics by group ---------------------------------------------------------------------------------------
BOX_CAP_FIRST = 65536                                              # boxes the first call has room for; more groups: one more call


def _ints(x, dtype, what):
    a = np.asarray(x)
    if a.size == 0:
        a = a.astype(dtype)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise TypeError("%s: a 1-D integer array is needed, not %s%s" % (what, a.dtype, list(a.shape)))
    if a.dtype != dtype:
        info = np.iinfo(dtype)
        if a.size and (int(a.min()) < info.min or int(a.max()) > info.max):
            raise ValueError("%s does not fit %s" % (what, np.dtype(dtype).name))
        a = a.astype(dtype)
    return np.ascontiguousarray(a)


def box_stats_raw(key, thou, interval: float = 0.0, whis: float = 1.5, device: int = 0, lib=None, box_cap=None):
    """lqfig_boxstats as it is: -> (sorted: the int32 thousandths group by group, inside a group ascending and the MISSING ones last;
    boxes: a BOX record per group that occurs, ascending in group).  box_cap: room for the boxes, default as many as needed"""
    k, t = _ints(key, np.uint32, "key"), _ints(thou, np.int32, "thou")
    if k.shape != t.shape:
        raise ValueError("one value per key")
    lib, n = _box_lib(lib), k.size
    out = np.empty(n, dtype=np.int32)
    cap = min(n, BOX_CAP_FIRST) if box_cap is None else int(box_cap)
    while True:
        boxes, nb, err = np.zeros(cap, dtype=BOX), C.c_uint32(0), C.create_string_buffer(512)
        rc = lib.lqfig_boxstats(device, _ptr(k), _ptr(t), n, float(interval), float(whis), _ptr(out), _ptr(boxes), cap, C.byref(nb), err, 512)
        if rc == -1 and box_cap is None and nb.value > cap:            # (LQCOV_E_ARG with the number of groups: once more with room for them)
            cap = nb.value
            continue
        _check(rc, err)
        return out, boxes[:nb.value]


def box_stats(key, thou, interval: float = 0.0, whis: float = 1.5, device: int = 0, lib=None) -> dict:
    """matplotlib.cbook.boxplot_stats(x, whis) of every group's non-missing values, on the device (kernels_boxstats.hpp).  thou: the values as
    printed "%.3f" numbers, integer thousandths (MISSING: "-nan"), their doubles thou / 1000; the group of element i is key[i], or with an
    interval np.floor(key[i] / interval).  -> a dict of arrays with one entry per group that occurs, ascending in group: group, n_all
    (members), n (non-missing members), q1, med, q3, whislo, whishi (np.percentile's linear rule; NaN for a group without values), median
    (np.median's and pandas': the mean of the two middle values, which can differ from med in the last bit), and fliers, a list of arrays:
    the values below whislo, then those above whishi, ascending"""
    s, b = box_stats_raw(key, thou, interval, whis, device, lib)
    out = {f: b[f].copy() for f in ("group", "n_all", "n", "q1", "med", "q3", "whislo", "whishi")}
    some = b["n"] > 0
    with np.errstate(invalid="ignore"):
        out["median"] = np.where(some, (b["mid_lo"] / 1000.0 + b["mid_hi"] / 1000.0) / 2, np.nan)
    out["fliers"] = [np.concatenate([s[f:f + lo], s[f + n - hi:f + n]]) / 1000.0
                     for f, n, lo, hi in zip(b["first"].astype(np.int64).tolist(), b["n"].astype(np.int64).tolist(), b["n_low"].astype(np.int64).tolist(), b["n_high"].astype(np.int64).tolist())]
    return out


_MASKED_EDGES = np.arange(0, 1.0, 0.01)                            # lq_mask.py:70



def masked_bin_table() -> np.ndarray:
    """the bin of each printed fraction k / 1000, k = 0 .. 1000, among np.arange(0, 1.0, 0.01), by numpy's own comparisons (np.histogram
    places a value with searchsorted on the edge array; the last bin is closed); 99: counted nowhere (above the last edge, 0.99).  No bin
    arithmetic: the edges are not k / 100 (edge 57 is 0.5700000000000001, so a printed 0.570 lies in the bin below)"""
    v = np.arange(1001) / 1000
    b = np.searchsorted(_MASKED_EDGES, v, side="right") - 1
    b[v == _MASKED_EDGES[-1]] = _MASKED_EDGES.size - 2
    b[v > _MASKED_EDGES[-1]] = 99
    return b.astype(np.int64)


_MASKED_BIN = masked_bin_table()


def masked_fraction_hist(frac_thou, device: int = 0, lib=None):
    """np.histogram(fractions, bins=np.arange(0, 1.0, 0.01)) of the masked-fraction figure (lq_mask.py:70) from the printed fractions as
    uint32 thousandths (0xffffffff: "-nan", counted nowhere) -> (edges, counts).  The device counts the 1001 possible values (lqfig_hist
    with the unit edges 0 .. 1001); masked_bin_table folds them into the figure's 99 bins"""
    a, _ = _values(frac_thou, U32)
    per_value = hist(a, np.arange(1002, dtype=np.float64), device, lib)
    counts = np.zeros(100, dtype=np.int64)
    np.add.at(counts, _MASKED_BIN, per_value)
    return _MASKED_EDGES.copy(), counts[:99]


# ---- the gamma fit ------------------------------------------------------------------------------------------------------
_PREC = 50                                                         # decimal digits of the solve
_SHIFT = 40                                                        # the asymptotic series are used from here on: term k falls like (k / (pi e y)) ** 2k


def _bernoulli_even(count):
    """B_2, B_4, ... as Fractions, from the recurrence sum_{k<=m} C(m + 1, k) B_k = 0"""
    B = [Fraction(1), Fraction(-1, 2)]
    for m in range(2, 2 * count + 1):
        B.append(-sum(math.comb(m + 1, k) * B[k] for k in range(m)) / (m + 1))
    return [B[2 * k] for k in range(1, count + 1)]


_B2K = _bernoulli_even(16)


def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


def _psi(x: Decimal) -> Decimal:
    """digamma(x), x > 0: psi(x) = psi(x + 1) - 1 / x up to _SHIFT, then ln y - 1 / 2y - sum B_2k / (2k y^2k)"""
    acc = Decimal(0)
    while x < _SHIFT:
        acc -= 1 / x
        x += 1
    y2, p = x * x, Decimal(1)
    acc += x.ln() - 1 / (2 * x)
    for k, b in enumerate(_B2K, 1):
        p *= y2
        acc -= _dec(b) / (2 * k * p)
    return acc


def _psi1(x: Decimal) -> Decimal:
    """trigamma(x), x > 0: psi1(x) = psi1(x + 1) + 1 / x^2 up to _SHIFT, then 1 / y + 1 / 2y^2 + sum B_2k / y^(2k+1)"""
    acc = Decimal(0)
    while x < _SHIFT:
        acc += 1 / (x * x)
        x += 1
    y2, p = x * x, x
    acc += 1 / x + 1 / (2 * y2)
    for b in _B2K:
        p *= y2
        acc += _dec(b) / p
    return acc


def digamma(x: float) -> float:
    if not x > 0 or not math.isfinite(x):
        raise ValueError("digamma is evaluated for positive finite x here")
    with localcontext() as ctx:
        ctx.prec = _PREC
        return float(_psi(Decimal(x)))


def trigamma(x: float) -> float:
    if not x > 0 or not math.isfinite(x):
        raise ValueError("trigamma is evaluated for positive finite x here")
    with localcontext() as ctx:
        ctx.prec = _PREC
        return float(_psi1(Decimal(x)))


def gamma_shape(s: float) -> float:
    """the root a of log(a) - digamma(a) = s, s > 0, as the nearest double: Newton's iteration at _PREC digits.  g(a) = log a - psi(a)
    falls and is convex, so from the left of the root the iterates rise towards it and never pass it; a start on the right lands on the
    left after one step, and a step that would leave a > 0 is replaced by halving"""
    if not s > 0 or not math.isfinite(s):
        raise ValueError("log(mean) - mean(log) must be positive and finite, not %r" % (s,))
    with localcontext() as ctx:
        ctx.prec = _PREC
        S = Decimal(s)
        a = Decimal((3 - s + math.sqrt((s - 3) ** 2 + 24 * s)) / (12 * s))        # Minka's start, the one scipy brackets around
        if not a > 0 or not a.is_finite():
            a = Decimal(1) / (2 * S)
        for _ in range(200):
            f = a.ln() - _psi(a) - S
            nxt = a - f / (1 / a - _psi1(a))
            if not nxt > 0:
                nxt = a / 2
            if abs(nxt - a) <= abs(nxt) * Decimal(10) ** -(_PREC - 10):
                return float(nxt)
            a = nxt
    raise ArithmeticError("the gamma shape iteration did not settle")


def gamma_fit(n: int, sum_x, sum_log: float):
    """scipy.stats.gamma.fit(x, floc=0) from the sums of x: n values, sum_x their sum, sum_log the sum of their logarithms -> (a, scale):
    the maximum-likelihood shape solves log(a) - digamma(a) = log(mean) - mean(log), scale = mean / a.  ValueError where the left side's
    value is not positive: no values, or values without spread (all equal: the likelihood grows with a without bound)"""
    if n < 1:
        raise ValueError("no values to fit")
    mean = sum_x / n
    if not mean > 0:
        raise ValueError("the values must be positive")
    s = math.log(mean) - sum_log / n
    a = gamma_shape(s)
    return a, mean / a

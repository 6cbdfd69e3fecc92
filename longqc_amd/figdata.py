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


def density_hist(x, start, stop, step, device: int = 0, lib=None):
    """-> (edges, counts, density): edges = np.arange(start, stop, step) whatever it yields, counts from hist, density = counts /
    np.diff(edges) / counts.sum(), numpy's expression and order: (density, edges) is np.histogram(x, bins=edges, density=True)"""
    edges = np.arange(start, stop, step)
    counts = hist(x, edges, device, lib)
    db = np.array(np.diff(edges), float)
    return edges, counts, counts / db / counts.sum()


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

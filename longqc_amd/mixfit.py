"""The two mixture fits behind LongQC's coverage estimate (lq_coverage.py:552-621) on the device, without sklearn and mixEM: gmm2 is
sklearn's GaussianMixture(n_components=2).fit of 1-D data from a deterministic start (the split of the sorted values with the smallest
two-cluster squared error, in place of the seeded k-means), lognorm_norm is mixem.em for a normal and a log-normal component.  Each fit
is one workgroup's whole EM loop in one launch (kernels_mixfit.hpp, behind lqmix_gmm2 / lqmix_lognorm of include/lqcov.h); the *_many
forms fit a list of arrays in one launch.  No CPU fallback: without liblqcov.so or a HIP device the calls raise.

A fit is a function of its values as a multiset: the same bytes whatever the order of the rows, the batch and the run."""
import ctypes as C

import numpy as np

from . import api

MAX_N = 9216                                                       # LQMIX_MAX_N
EXIT_TOL, EXIT_MAX, EXIT_NAN = 0, 1, 2                             # LQMIX_EXIT_*
EXITS = ("tol", "max", "nan")
# lqmix_fit of include/lqcov.h
FIT = np.dtype([("w", np.float64, 2), ("mu", np.float64, 2), ("s", np.float64, 2), ("ll", np.float64), ("n_iter", np.uint32),
                ("exit", np.uint32), ("n", np.uint64)])
assert FIT.itemsize == 72


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqmix_bound", False):
        tail = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lqmix_gmm2.restype = lib.lqmix_lognorm.restype = C.c_int
        lib.lqmix_gmm2.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.c_double] + tail
        lib.lqmix_lognorm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32] + tail
        lib._lqmix_bound = True
    return lib


def _segments(arrays):
    """a list of 1-D arrays -> (their float64 values one after the other, the uint64 offsets)"""
    parts = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    if any(p.ndim != 1 for p in parts):
        raise TypeError("every fit takes a 1-D array")
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0)), off


def _check(rc, err):
    if rc != 0:
        raise api.LqcovError(rc, err.value.decode())


def _ptr(a):
    return a.ctypes.data if a.size else None


def _dicts(fits, second):
    return [{"w": f["w"].copy(), "mu": f["mu"].copy(), second: f["s"].copy(), "ll": float(f["ll"]), "n_iter": int(f["n_iter"]),
             "exit": EXITS[int(f["exit"])], "n": int(f["n"])} for f in fits]


def gmm2_raw(arrays, tol=1e-3, max_iter=100, reg_covar=1e-6, device: int = 0, lib=None) -> np.ndarray:
    """lqmix_gmm2 as it is: one FIT record per array"""
    x, off = _segments(arrays)
    out, err = np.zeros(len(arrays), dtype=FIT), C.create_string_buffer(512)
    _check(_lib(lib).lqmix_gmm2(device, _ptr(x), off.ctypes.data, len(arrays), float(tol), int(max_iter), float(reg_covar), _ptr(out), err, 512), err)
    return out


def lognorm_norm_raw(arrays, inits, tol=1e-15, tol_iters=10, max_iter=500, device: int = 0, lib=None) -> np.ndarray:
    """lqmix_lognorm as it is: one FIT record per array; inits: per array (mu_bg, sigma_bg, mu_logn, sigma_logn)"""
    x, off = _segments(arrays)
    init = np.ascontiguousarray(inits, dtype=np.float64).reshape(-1)
    if init.size != 4 * len(arrays):
        raise ValueError("four starting numbers per fit")
    out, err = np.zeros(len(arrays), dtype=FIT), C.create_string_buffer(512)
    _check(_lib(lib).lqmix_lognorm(device, _ptr(x), off.ctypes.data, len(arrays), _ptr(init), float(tol), int(tol_iters), int(max_iter), _ptr(out),
                                   err, 512), err)
    return out


def gmm2_many(arrays, tol=1e-3, max_iter=100, reg_covar=1e-6, device: int = 0, lib=None) -> list:
    """sklearn's two-component GaussianMixture.fit of every array, in one launch -> per array a dict: w, mu, var (arrays of 2, the
    components ascending in mean), ll (the last lower bound), n_iter, exit ("tol" / "max"), n.  Each array has 2 .. MAX_N finite values
    that are not all equal (LqcovError otherwise)"""
    return _dicts(gmm2_raw(arrays, tol, max_iter, reg_covar, device, lib), "var")


def gmm2(x, tol=1e-3, max_iter=100, reg_covar=1e-6, device: int = 0, lib=None) -> dict:
    return gmm2_many([x], tol, max_iter, reg_covar, device, lib)[0]


def lognorm_norm_many(arrays, inits, tol=1e-15, tol_iters=10, max_iter=500, device: int = 0, lib=None) -> list:
    """mixem.em(x, [NormalDistribution(mu_bg, sigma_bg), LogNormalDistribution(mu_logn, sigma_logn)], max_iterations=max_iter) of every
    array, in one launch -> per array a dict: w, mu, sigma (component 0 the normal, 1 the log-normal), ll, n_iter (passes made), exit
    ("tol" / "max" / "nan": a NaN log-likelihood is reported, not raised), n.  The values are positive"""
    return _dicts(lognorm_norm_raw(arrays, inits, tol, tol_iters, max_iter, device, lib), "sigma")


def lognorm_norm(x, init, tol=1e-15, tol_iters=10, max_iter=500, device: int = 0, lib=None) -> dict:
    return lognorm_norm_many([x], [init], tol, tol_iters, max_iter, device, lib)[0]


def main_component(fit) -> int:
    """the index of the coverage component of a gmm2 fit: the largest w / var, the first of equals (lq_coverage.py:591-606)"""
    order = np.asarray(fit["w"]) / np.asarray(fit["var"])
    return 1 if order[0] < order[1] else 0

"""The histograms of the GC figure and the length figure (k_fig_hist / k_fig_range of kernels_figdata.hpp behind lqfig_hist / lqfig_range;
figdata.hist, figdata.value_range, figdata.density_hist) under the wave emulator and on the GPU: edges, counts and density are compared
for exact equality with np.histogram(x, bins=np.arange(...), density=True), which the test runs itself.

Which case notices which slip:
  the last bin half-open              "dyadic edges" (a value equal to the last edge), "lengths, span a multiple of the width" (the longest
                                      read is the last edge).  Built once, below: test_a_half_open_last_bin_is_noticed names the cases.
  `<` where numpy has `<=`            "dyadic edges" (a value on every inner edge goes right), "lengths, span a multiple of the width"
                                      (lengths on the inner edges)
  bins from e0 + k w, not the edges   "uneven edges" (no width describes them); for np.arange's edges the two differ by an ulp of a double,
                                      which no float32 value lies between, and for integers not at all -- the edge array still decides
  float32 compared as float32         "around every edge": the float32 neighbours of each edge of np.arange(0.31, 0.71, 0.02); an edge rounded
                                      to float32 moves onto or past one of them (about half the edges round down, onto the value below)
  NaN or outside values counted       "around every edge" (one value below the first edge, the successor of the last edge, a NaN)
  counters of a second round lost     "past the launch cap" (3 bins, LQ_FIG_MAX_BLOCKS * LQ_FIG_THREADS + 300 values)
  the global path's edges or atomics  "one bin more than LDS holds" (LQ_FIG_HIST_LDS_BINS + 1 bins)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from longqc_amd import api
from longqc_amd import figdata as F
from tests import test_figdata_kde as TK
from tests import test_launch_caps as LC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "longqc_amd", "csrc")


def same_as_numpy(x, start, stop, step, lib, what):
    edges, counts, density = F.density_hist(x, start, stop, step, lib=lib)
    want_edges = np.arange(start, stop, step)
    with np.errstate(all="ignore"):
        want_density, e2 = np.histogram(x, bins=want_edges, density=True)
        want_counts, _ = np.histogram(x, bins=want_edges)
    assert edges.dtype == want_edges.dtype and edges.tobytes() == want_edges.tobytes(), what
    assert counts.tolist() == want_counts.tolist(), (what, counts, want_counts)
    assert density.dtype == want_density.dtype and density.tobytes() == want_density.tobytes(), (what, density, want_density)
    return counts


def around_every_edge():
    """-> (float32 values, edges): for every edge e of np.arange(0.31, 0.71, 0.02) the float32 below e, the one at or above it and the
    neighbour of each; the successor's successor of the last edge, one value below the first edge, a NaN"""
    edges = np.arange(0.31, 0.71, 0.02)
    vals = []
    for e in edges.tolist():
        f = np.float32(e)
        below = f if float(f) < e else np.nextafter(f, np.float32(-np.inf))
        above = np.nextafter(below, np.float32(np.inf))
        assert float(below) < e <= float(above)
        vals += [np.nextafter(below, np.float32(-np.inf)), below, above, np.nextafter(above, np.float32(np.inf))]
    vals += [np.float32(0.2), np.float32(np.nan)]
    x = np.array(vals, dtype=np.float32)
    assert (edges.astype(np.float32).astype(np.float64) < edges).sum() >= 5 and (edges.astype(np.float32).astype(np.float64) > edges).sum() >= 5
    return x, edges


def dyadic_edges():
    """edges 0.25, 0.375 .. 0.75, every one a float32: the edge itself, its predecessor and successor, for every edge"""
    edges = np.arange(0.25, 0.875, 0.125)
    assert edges.tolist() == [0.25, 0.375, 0.5, 0.625, 0.75]
    vals = []
    for e in edges.astype(np.float32):
        vals += [np.nextafter(e, np.float32(-np.inf)), e, e, np.nextafter(e, np.float32(np.inf))]
    return np.array(vals, dtype=np.float32), edges


def length_cases():
    cap, block, lds = LC.header_define("LQ_FIG_MAX_BLOCKS"), LC.header_define("LQ_FIG_THREADS"), LC.header_define("LQ_FIG_HIST_LDS_BINS")
    rng = np.random.default_rng(21)
    n_cap = cap * block + 300
    LC.assert_past_cap("k_fig_hist, values", n_cap, cap * block, block)
    wide = rng.integers(120, 120 + 1000 * (lds + 1), 6000)
    wide[:2] = (120, 120 + 1000 * (lds + 1) - 1)
    out = {"one read": np.array([4321]), "all equal": np.full(40, 1500),
           "lengths, span a multiple of the width": np.array([500, 1500, 1500, 2499, 2500, 3499, 3500, 3500, 501, 1499]),
           "gamma-like": np.array(TK.CASES["lengths"][0]["lengths"]),
           "one bin more than LDS holds": wide,
           "past the launch cap": np.concatenate([[77, 3076], rng.integers(77, 3077, n_cap - 2)])}
    assert (out["lengths, span a multiple of the width"].max() - out["lengths, span a multiple of the width"].min()) % 1000 == 0
    assert np.arange(120, wide.max() + 1000, 1000).shape[0] - 1 == lds + 1
    assert np.arange(77, 3076 + 1000, 1000).shape[0] - 1 == 3
    return {k: v.astype(np.uint32) for k, v in out.items()}


def check_gc_cases(lib):
    for case in TK.CASES["kde"]:
        x = TK.fractions_of(case)
        lo, hi = F.value_range(x, lib=lib)
        assert lo == x.min() and hi == x.max() and lo.dtype == np.float32
        c = same_as_numpy(x, float(lo), float(hi) + 0.02, 0.02, lib, case["name"])
        assert c.sum() == case["n"]                                  # min and max + b_width are the edges: every value is counted


def check_edge_sets(lib):
    x, edges = around_every_edge()
    got = F.hist(x, edges, lib=lib)
    want, _ = np.histogram(x, bins=edges)
    assert got.tolist() == want.tolist() and got.dtype == np.int64, ("around every edge", got, want)
    assert got.sum() == x.shape[0] - 2 - 2 - 2                       # the first edge's two lower values, the last edge's two upper ones, 0.2, NaN
    c = same_as_numpy(x, 0.31, 0.71, 0.02, lib, "around every edge")
    assert c.tolist() == want.tolist()
    x, edges = dyadic_edges()
    got = F.hist(x, edges, lib=lib)
    assert got.tolist() == np.histogram(x, bins=edges)[0].tolist() == [4, 4, 4, 4 + 2], ("dyadic edges", got)
    same_as_numpy(x, 0.25, 0.875, 0.125, lib, "dyadic edges")
    uneven = np.array([0.0, 0.1, 0.5, 0.55, 1.0])
    x = np.random.default_rng(4).random(2000).astype(np.float32)
    got = F.hist(x, uneven, lib=lib)
    assert got.tolist() == np.histogram(x, bins=uneven)[0].tolist() and got.sum() == 2000, ("uneven edges", got)
    assert F.value_range(np.array([np.nan, 0.5, -0.0, -3.0, np.nan], dtype=np.float32), lib=lib) == (-3.0, 0.5)


def check_lengths(lib):
    for what, lens in length_cases().items():
        lo, hi = F.value_range(lens, lib=lib)
        assert lo == lens.min() and hi == lens.max() and lo.dtype == np.uint32, what
        c = same_as_numpy(lens, int(lo), int(hi) + 1000, 1000, lib, what)
        if what in ("one read", "all equal"):
            assert c.shape == (0,)                                  # np.arange(min, min + 1000, 1000) is one edge: no bin
        else:
            assert c.sum() == lens.shape[0], what
    big = np.array([2 ** 32 - 1, 0, 2 ** 31], dtype=np.uint32)
    assert F.value_range(big, lib=lib) == (0, 2 ** 32 - 1)
    assert F.hist(big, [0, 2 ** 31, 2 ** 32 - 1], lib=lib).tolist() == [1, 2]


def check_no_bins_and_refusals(lib):
    x = np.array([0.25, 0.5], dtype=np.float32)
    for edges in ([], [0.3]):
        got = F.hist(x, edges, lib=lib)
        assert got.shape == (0,) and got.dtype == np.int64
    assert F.hist(np.zeros(0, np.float32), [0.0, 0.5, 1.0], lib=lib).tolist() == [0, 0]      # n == 0 is no error
    for edges in ([0.5, 0.25], [0.0, 0.5, 0.4, 1.0], [0.0, np.nan]):
        with pytest.raises(api.LqcovError) as e:
            F.hist(x, edges, lib=lib)
        assert e.value.code == -1                                   # LQCOV_E_ARG, where numpy raises ValueError
    assert F.hist(x, [0.0, 0.5, 0.5, 1.0], lib=lib).tolist() == np.histogram(x, bins=[0.0, 0.5, 0.5, 1.0])[0].tolist()      # (equal neighbours pass, as in numpy)
    with pytest.raises(ValueError):
        F.value_range(np.zeros(0, np.float32), lib=lib)
    with pytest.raises(TypeError):
        F.hist(np.array([1, 2], dtype=np.int64), [0, 5], lib=lib)


def check_all(lib):
    check_gc_cases(lib)
    check_edge_sets(lib)
    check_lengths(lib)
    check_no_bins_and_refusals(lib)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_histograms_are_numpys(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_all(emu_lib)


def test_a_half_open_last_bin_is_noticed(emu_lib, tmp_path):
    """figdata.cpp built again for the emulator with LQ_FIG_LAST_BIN_CLOSED=0 (the rest of the library comes from the session's build):
    "dyadic edges" and "lengths, span a multiple of the width" fail -- the values on the last edge are lost -- and no other case does"""
    so = str(tmp_path / "liblqfig_half_open.so")
    emu = os.path.join(ROOT, "tests", "emu")
    r = subprocess.run(["g++", "-DLQ_EMU", "-DLQ_FIG_LAST_BIN_CLOSED=0", "-include", os.path.join(emu, "hipemu.hpp"), "-O1", "-std=c++17", "-fPIC",
                        "-Wno-unknown-pragmas", "figdata.cpp", "-shared", "-o", so, os.path.join(emu, "liblqcov_emu.so"), "-Wl,-rpath," + emu, "-lz"],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    lib = C.CDLL(so)
    x, edges = dyadic_edges()
    assert F.hist(x, edges, lib=lib).tolist() == [4, 4, 4, 4] and F.hist(x, edges, lib=emu_lib).tolist() == [4, 4, 4, 6]
    lens = length_cases()["lengths, span a multiple of the width"]
    e = np.arange(500, 3500 + 1000, 1000)
    assert F.hist(lens, e, lib=lib).sum() == lens.shape[0] - 2 and F.hist(lens, e, lib=emu_lib).sum() == lens.shape[0]
    with pytest.raises(AssertionError):
        check_edge_sets(lib)
    with pytest.raises(AssertionError):
        check_lengths(lib)
    check_gc_cases(lib)                                            # (their last edge lies above the maximum)
    x, edges = around_every_edge()
    assert F.hist(x, edges, lib=lib).tolist() == np.histogram(x, bins=edges)[0].tolist()


@pytest.mark.gpu
def test_gpu_histograms_are_numpys(gpu_lib):
    check_all(gpu_lib)

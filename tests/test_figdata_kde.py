"""The KDE curves of the GC figure (k_fig_kde / k_fig_fold of kernels_figdata.hpp behind lqfig_kde; figdata.kde_sums,
figdata.gaussian_kde_curve) under the wave emulator and on the GPU, against tests/golden/figdata_cases.json (written by
tests/golden/make_figdata_golden.py with scipy and decimal at 60 digits):

  1. against the exact density: |got - exact| <= tol[j] * exact where exact >= 1e-300, <= 1e-300 absolute below that, exactly 0 where
     the exact value lies below 2^-1075; tol[j] is the file's first-order bound (3 t_i + 300 units of 2^-53 per term);
  2. against scipy's recorded curve where exact >= 1e-6 * max: relative difference <= tol[j] + (12 / h + n) 2^-53 -- scipy whitens
     first (p / h - d / h: an absolute error of about 2^-53 / h in u, times |u| <= 6 in the exponent) and adds sequentially;
  3. determinism: the same case under every thread order of the emulator, twice on the GPU, and with the launch cut to one block
     (LQFIG_TEST_MAX_BLOCKS=1, read at every call) gives byte-identical doubles;
  4. shapes: m = 1, 50, 65 (one point, the figure's, one past a wave's 64 lanes) x n = 2, 255, 256, 257 (around one tile), and constant
     data past the launch cap (256 * LQ_FIG_MAX_BLOCKS * 4 + 300 values: the first waves take a second tile, the last tile is partial);
  5. refusals: h = 0, h = nan, m = 0 (LQCOV_E_ARG); one value and values without variance through gaussian_kde_curve (ValueError);
  6. where scipy is importable: its curve for one case, regenerated, is the file's: the golden file is pinned to the library."""
import json
import math
import os

import numpy as np
import pytest

from longqc_amd import api
from longqc_amd import figdata as F
from tests import test_launch_caps as LC
from tests.conftest import GOLDEN

EPS = 2.0 ** -53
CASES = json.load(open(os.path.join(GOLDEN, "figdata_cases.json")))
XS = np.array([float.fromhex(v) for v in CASES["points"]])
KDE = {c["name"]: c for c in CASES["kde"]}


def unhex(vals):
    return np.array([float.fromhex(v) for v in vals])


def fractions_of(case):
    x = np.frombuffer(bytes.fromhex(case["x_f32_hex"]), dtype=">u4").astype(np.uint32).view(np.float32)
    assert x.shape[0] == case["n"]
    return x


def test_the_points_are_the_figures():
    assert XS.tobytes() == np.linspace(0, 1.0, 50).tobytes()
    first = unhex(KDE["gc_cloud"]["exact"])
    assert (first == 0).sum() >= 1 and ((first > 1e-300) & (first < 1e-200)).any() and (first > 1e-6 * first.max()).sum() >= 3
    assert sorted(np.flatnonzero(first == 0).tolist()) == KDE["gc_cloud"]["underflow"]
    assert [KDE[k]["n"] for k in ("two_values", "one_past_a_tile", "one_past_two_tiles")] == [2, LC.header_define("LQ_FIG_TILE") + 1, 2 * LC.header_define("LQ_FIG_TILE") + 1]


def check_golden_curves(lib):
    worst_exact = worst_scipy = 0.0
    for case in CASES["kde"]:
        x, h, n = fractions_of(case), float.fromhex(case["h"]), case["n"]
        got, got_h = F.gaussian_kde_curve(x, XS, lib=lib, return_bandwidth=True)
        assert got_h == h, (case["name"], got_h.hex(), case["h"])      # the bandwidth is scipy's number, not a tolerance question
        exact, tol, sp = unhex(case["exact"]), unhex(case["tol"]), unhex(case["scipy"])
        for j in range(50):
            if j in case["underflow"]:
                assert got[j] == 0.0, (case["name"], j, got[j])
            elif exact[j] < 1e-300:
                assert abs(got[j] - exact[j]) <= 1e-300, (case["name"], j, got[j], exact[j])
            else:
                r = abs(got[j] - exact[j]) / (tol[j] * exact[j])
                worst_exact = max(worst_exact, r)
                assert r <= 1, (case["name"], j, got[j], exact[j], tol[j])
        near = np.flatnonzero(exact >= 1e-6 * exact.max())
        assert near.shape[0] >= 3
        bound = tol[near] + (12 / h + n) * EPS
        r = np.abs(got[near] - sp[near]) / exact[near] / bound
        worst_scipy = max(worst_scipy, float(r.max()))
        assert (r <= 1).all(), (case["name"], near[r > 1], got[near][r > 1], sp[near][r > 1])
    print("largest error / bound: %.4f against the exact density, %.4f against scipy's curve" % (worst_exact, worst_scipy))


def terms_of(x, p, h):
    u = (np.asarray(p, dtype=np.float64)[:, None] - np.asarray(x).astype(np.float64)[None, :]) / h
    t = 0.5 * u * u
    return t, np.exp(-t)


def first_order_tol(x, p, h, per_t=3, fixed=300):
    """the golden file's tol[j] from the terms in double: sum_i term_i (3 t_i + 300) 2^-53 / sum_i term_i (0 where the sum is 0)"""
    t, term = terms_of(x, p, h)
    s = np.array([math.fsum(row) for row in term])
    w = np.array([math.fsum(row) for row in term * (per_t * t + fixed)])
    return np.where(s > 0, w / np.where(s > 0, s, 1), 0) * EPS


def model_sums(x, p, h):
    """-> (sums, bound): the terms exp(-0.5 u u), u = (p - d) / h, in double with numpy and math.fsum over them, and the bound on
    |kernel - model| relative to the sum: the kernel's 3 t + 300 units of 2^-53 per term (the golden file's tol) plus the model's own
    3 t + 3 (the same three roundings in front of exp, one ulp = two units of numpy's exp, fsum's one rounding)"""
    _, term = terms_of(x, p, h)
    return np.array([math.fsum(row) for row in term]), first_order_tol(x, p, h, 6, 303)


def check_shapes(lib):
    rng = np.random.default_rng(5)
    for n in (2, 255, 256, 257):
        x = rng.beta(8, 12, n).astype(np.float32)
        for m in (1, 50, 65):
            p = np.linspace(0.05, 0.95, m) if m > 1 else np.array([0.4])
            got = F.kde_sums(x, p, 0.03, lib=lib)
            want, bound = model_sums(x, p, 0.03)
            assert got.shape == (m,) and (want > 0).all()
            assert (np.abs(got - want) <= bound * want).all(), (n, m, got, want)
    assert F.kde_sums(np.zeros(0, np.float32), [0.1, 0.2], 0.5, lib=lib).tolist() == [0.0, 0.0]      # n == 0 is no error: S[j] = 0


def check_past_cap(lib):
    cap, tile, waves = LC.header_define("LQ_FIG_MAX_BLOCKS"), LC.header_define("LQ_FIG_TILE"), LC.header_define("LQ_FIG_THREADS") // 64
    n = tile * cap * waves + 300
    LC.assert_past_cap("k_fig_kde, values", n, tile * cap * waves, tile)
    d, h = np.float32(0.375), 0.25
    x = np.full(n, d, dtype=np.float32)
    p = np.array([0.375, 0.75, 0.375 + 40 * h])                    # u = 0, 1.5 and 40 (n exp(-800) is 0 in double)
    got = F.kde_sums(x, p, h, lib=lib)
    u = (p - float(d)) / h
    assert u.tolist() == [0.0, 1.5, 40.0]                            # (exact: the bound below has no 3 t part)
    want = n * np.exp(-0.5 * u * u)
    # the kernel's 300 units (one ulp of exp, 256 sequential additions, the tree's ceil(log2(tiles)) levels) and, here, one ulp of
    # numpy's exp and the product's rounding
    assert 2 + 256 + math.ceil(math.log2(n / tile)) <= 300
    bound = 303 * EPS
    assert got[2] == 0.0 and got[0] == float(n), got
    assert abs(got[1] - want[1]) <= bound * want[1], (got[1], want[1])


def check_refusals(lib):
    x = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    for h, pts in ((0.0, [0.5]), (math.nan, [0.5]), (-1.0, [0.5]), (math.inf, [0.5]), (0.1, [])):
        with pytest.raises(api.LqcovError) as e:
            F.kde_sums(x, pts, h, lib=lib)
        assert e.value.code == -1, (h, pts)                         # LQCOV_E_ARG
    with pytest.raises(ValueError):
        F.gaussian_kde_curve(x[:1], XS, lib=lib)
    with pytest.raises(ValueError):
        F.gaussian_kde_curve(np.full(9, 0.5, dtype=np.float32), XS, lib=lib)
    with pytest.raises(TypeError):
        F.kde_sums(x.astype(np.float64), [0.5], 0.1, lib=lib)


def curves(lib):
    out = []
    for name in ("gc_cloud", "one_past_two_tiles"):
        x = fractions_of(KDE[name])
        out.append(F.kde_sums(x, XS, float.fromhex(KDE[name]["h"]), lib=lib).tobytes())
    rng = np.random.default_rng(9)                                  # several tiles per wave of a one-block launch, m past a wave
    out.append(F.kde_sums(rng.random(256 * 9 + 17).astype(np.float32), np.linspace(0, 1, 65), 0.01, lib=lib).tobytes())
    return out


def test_emulated_golden_curves(emu_lib):
    check_golden_curves(emu_lib)


def test_emulated_curves_are_the_same_bytes_under_every_order_and_grid(emu_lib, monkeypatch):
    monkeypatch.delenv("LQFIG_TEST_MAX_BLOCKS", raising=False)
    seen = []
    for order in LC.ORDERS:
        LC.set_order(monkeypatch, order)
        seen.append(curves(emu_lib))
    monkeypatch.setenv("LQFIG_TEST_MAX_BLOCKS", "1")
    seen.append(curves(emu_lib))
    assert all(s == seen[0] for s in seen)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_shapes_and_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_shapes(emu_lib)
    check_past_cap(emu_lib)


def test_emulated_refusals(emu_lib):
    check_refusals(emu_lib)


def test_the_golden_curve_is_scipys():
    stats = pytest.importorskip("scipy.stats")
    case = KDE["one_past_a_tile"]
    k = stats.gaussian_kde(fractions_of(case))
    assert math.isclose(math.sqrt(float(k.covariance[0, 0])), float.fromhex(case["h"]), rel_tol=8 * EPS)
    assert np.allclose(k(XS), unhex(case["scipy"]), rtol=1e-12, atol=0)      # (another build of the library may round otherwise)


@pytest.mark.gpu
def test_gpu_golden_curves(gpu_lib):
    check_golden_curves(gpu_lib)


@pytest.mark.gpu
def test_gpu_curves_are_the_same_bytes_twice_and_on_one_block(gpu_lib, monkeypatch):
    monkeypatch.delenv("LQFIG_TEST_MAX_BLOCKS", raising=False)
    seen = [curves(gpu_lib), curves(gpu_lib)]
    monkeypatch.setenv("LQFIG_TEST_MAX_BLOCKS", "1")
    seen.append(curves(gpu_lib))
    assert all(s == seen[0] for s in seen)


@pytest.mark.gpu
def test_gpu_shapes_and_cap(gpu_lib):
    check_shapes(gpu_lib)
    check_past_cap(gpu_lib)


@pytest.mark.gpu
def test_gpu_refusals(gpu_lib):
    check_refusals(gpu_lib)

"""The sums and the fit behind Length_stats.gamma_params (k_fig_logsum / k_fig_fold behind lqfig_logsum; figdata.log_sums,
figdata.gamma_fit, LqMaskMI355X.length_figure_data) under the wave emulator and on the GPU.

  log_sums   sum x and the number of zeros are exact; sum log is within (2 + 256 + log2 n) 2^-53 sum |log x| of math.fsum(math.log(v)) -- a
             unit for each of the two logarithm functions, the sequential additions of a tile, the levels of the tree; n = 1, 257 and past
             the launch cap, the values 1 (log 0), 2 and 2^32 - 1 among them; byte-identical under every thread order of the emulator and
             with the launch cut to one block.
  gamma_fit  host only.  For the shapes 0.3, 1.0, 1.3, 8 and 200, from exact sums (mean 1, mean log -s, s the double nearest to log a -
             psi(a)): the residual |log a' - psi(a') - s| of the returned a', evaluated here with decimal at 60 digits (the recurrence up
             to 60 and the asymptotic series: no mpmath), is at most 8 * 2^-53 * max(1, |log a'|).
  the fit    length_figure_data()["gamma_params"] against the golden scipy.stats.gamma.fit(lengths, floc=0) to 1e-9 relative: brentq's
             xtol of 2e-12 on a, plus the sum's bound carried through s = log(mean) - mean log at these sets, with two orders of margin.
             Lengths with a zero, no reads, one read and equal reads raise ValueError (scipy raises it for the last two as well: the
             golden file records its exception)."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

from longqc_amd import figdata as F
from longqc_amd import sdust
from tests import test_figdata_kde as TK
from tests import test_launch_caps as LC

EPS = 2.0 ** -53
LENGTHS = {c["name"]: c for c in TK.CASES["lengths"]}


# ---- log_sums -----------------------------------------------------------------------------------------------------------
def sum_cases():
    cap, tile, waves = LC.header_define("LQ_FIG_MAX_BLOCKS"), LC.header_define("LQ_FIG_TILE"), LC.header_define("LQ_FIG_THREADS") // 64
    rng = np.random.default_rng(33)
    n_cap = tile * cap * waves + 300
    LC.assert_past_cap("k_fig_logsum, values", n_cap, tile * cap * waves, tile)
    special = np.array([1, 2, 2 ** 32 - 1, 1, 2 ** 32 - 1], dtype=np.uint32)
    big = rng.integers(1, 200000, n_cap).astype(np.uint32)
    big[[0, 5, tile * cap * waves + 7, n_cap - 1]] = (2 ** 32 - 1, 1, 2, 2 ** 32 - 1)
    return {"one value": np.array([12345], dtype=np.uint32), "one": np.array([1], dtype=np.uint32),
            "one past a tile": np.concatenate([special, rng.integers(1, 2 ** 32, tile + 1 - 5).astype(np.uint32)]),
            "gamma-like": np.array(LENGTHS["gamma_like"]["lengths"], dtype=np.uint32), "past the launch cap": big}


def check_log_sums(lib):
    out = []
    for what, x in sum_cases().items():
        total, sum_log, zeros = F.log_sums(x, lib=lib)
        n = x.shape[0]
        assert total == int(x.sum(dtype=np.uint64)) and zeros == 0, what
        logs = [math.log(v) for v in x.tolist()]
        want = math.fsum(logs)
        bound = (2 + 256 + math.log2(n)) * EPS * math.fsum(abs(v) for v in logs)
        print("%s: n %d, sum log %r, |error| %.3g of a bound of %.3g" % (what, n, sum_log, abs(sum_log - want), bound))
        assert abs(sum_log - want) <= bound, (what, sum_log, want)
        out.append(np.float64(sum_log).tobytes())
    assert F.log_sums(np.array([1], dtype=np.uint32), lib=lib) == (1, 0.0, 0)
    total, sum_log, zeros = F.log_sums(np.array([0, 7, 0, 0, 2], dtype=np.uint32), lib=lib)                           # zeros are counted, not added
    assert (total, zeros) == (9, 3) and abs(sum_log - math.log(14)) <= 6 * EPS * math.log(14)
    assert F.log_sums(np.zeros(0, np.uint32), lib=lib) == (0, 0.0, 0)                                               # n == 0 is no error
    with pytest.raises(TypeError):
        F.log_sums(np.array([1.0], dtype=np.float32), lib=lib)
    return out


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_log_sums(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_log_sums(emu_lib)


def test_emulated_log_sums_are_the_same_bytes_under_every_order_and_grid(emu_lib, monkeypatch):
    monkeypatch.delenv("LQFIG_TEST_MAX_BLOCKS", raising=False)
    seen = []
    for order in LC.ORDERS:
        LC.set_order(monkeypatch, order)
        seen.append(check_log_sums(emu_lib))
    monkeypatch.setenv("LQFIG_TEST_MAX_BLOCKS", "1")
    seen.append(check_log_sums(emu_lib))
    assert all(s == seen[0] for s in seen)


@pytest.mark.gpu
def test_gpu_log_sums(gpu_lib, monkeypatch):
    monkeypatch.delenv("LQFIG_TEST_MAX_BLOCKS", raising=False)
    seen = [check_log_sums(gpu_lib), check_log_sums(gpu_lib)]
    monkeypatch.setenv("LQFIG_TEST_MAX_BLOCKS", "1")
    seen.append(check_log_sums(gpu_lib))
    assert all(s == seen[0] for s in seen)


# ---- gamma_fit, host only -----------------------------------------------------------------------------------------------
def bernoulli(m_max):
    B = [Fraction(1)]
    for m in range(1, m_max + 1):
        B.append(-sum(math.comb(m + 1, k) * B[k] for k in range(m)) / (m + 1))
    return B


BERNOULLI = bernoulli(40)


def g_exact(a: Decimal) -> Decimal:
    """log(a) - digamma(a) at the context's precision: digamma(a) = digamma(a + N) - sum_{k<N} 1 / (a + k) with a + N >= 60, and
    digamma(y) = ln y - 1 / 2y - sum_k B_2k / (2k y^2k), whose 20th term is below 1e-45 there"""
    acc, y = Decimal(0), a
    while y < 60:
        acc += 1 / y
        y += 1
    series = 1 / (2 * y)
    for k in range(1, 21):
        b = BERNOULLI[2 * k]
        series += Decimal(b.numerator) / Decimal(b.denominator) / (2 * k * y ** (2 * k))
    return a.ln() - y.ln() + series + acc


def test_the_high_precision_digamma_knows_its_constants():
    with localcontext() as ctx:
        ctx.prec = 60
        euler = Decimal("0.577215664901532860606512090082402431042159335939923598805767")
        assert abs(g_exact(Decimal(1)) - euler) < Decimal("1e-45")                          # psi(1) = -gamma
        ln2 = Decimal(2).ln()
        assert abs(g_exact(Decimal("0.5")) - (-ln2 + euler + 2 * ln2)) < Decimal("1e-45")     # psi(1/2) = -gamma - 2 ln 2


@pytest.mark.parametrize("shape", [0.3, 1.0, 1.3, 8.0, 200.0])
def test_gamma_fit_solves_its_equation_to_the_last_bits(shape):
    with localcontext() as ctx:
        ctx.prec = 60
        s = float(g_exact(Decimal(shape)))
        a, scale = F.gamma_fit(1, 1, -s)                               # mean 1, mean log -s: log(mean) - mean log is s exactly
        resid = abs(g_exact(Decimal(a)) - Decimal(s))
        bound = 8 * EPS * max(1.0, abs(math.log(a)))
        print("shape %r: a %r, residual %.3g of a bound of %.3g" % (shape, a, float(resid), bound))
        assert resid <= Decimal(bound)
    assert abs(a - shape) <= 1e-12 * shape and scale == 1 / a
    assert F.gamma_fit(7, 7 * 2500, 7 * (math.log(2500) - s)) == pytest.approx((a, 2500 / a), rel=1e-10)


def test_gamma_fit_refuses_what_has_no_maximum():
    for n, sx, sl in ((0, 0, 0.0), (3, 0, 0.0), (1, 5, math.log(5)), (4, 28, 4 * math.log(7))):
        with pytest.raises(ValueError):
            F.gamma_fit(n, sx, sl)
    assert F.digamma(1.0) == pytest.approx(-0.5772156649015329, rel=1e-15) and F.trigamma(1.0) == pytest.approx(math.pi ** 2 / 6, rel=1e-15)


# ---- the fit of a mask's lengths ----------------------------------------------------------------------------------------
def mask_of(lens, lib, tmp_path, chunks=3):
    m = sdust.LqMaskMI355X(str(tmp_path), lib=lib)
    lens = np.asarray(lens, dtype=np.int64)
    for k, part in enumerate(np.array_split(lens, chunks)):
        m._note(k, part, 0, 0, [], [])                              # (what submit_sdust keeps of a chunk: its lengths)
    return m


def check_length_figure(lib, tmp_path):
    case = LENGTHS["gamma_like"]
    lens = np.array(case["lengths"], dtype=np.int64)
    m = mask_of(lens, lib, tmp_path)
    d = m.length_figure_data()
    a, scale = d["gamma_params"]
    want_a, want_scale = (float.fromhex(v) for v in case["gamma_fit"])
    print("a %r against scipy's %r (%.3g relative), scale %r against %r" % (a, want_a, abs(a - want_a) / want_a, scale, want_scale))
    assert abs(a - want_a) <= 1e-9 * want_a and abs(scale - want_scale) <= 1e-9 * want_scale
    edges = np.arange(lens.min(), lens.max() + 1000, 1000)
    want_density, _ = np.histogram(lens, bins=edges, density=True)
    assert d["hist"][0].tobytes() == edges.tobytes() and d["hist"][2].tobytes() == want_density.tobytes()
    s = m.summary()
    assert (d["mean_length"], d["n50"], d["longest"]) == (s["mean_length"], s["n50"], s["longest"])
    for name in ("one_read", "all_equal"):                          # scipy hands brentq s = 0 there and raises ValueError too
        assert "ValueError" in LENGTHS[name]["gamma_fit_raises"]
        with pytest.raises(ValueError):
            mask_of(LENGTHS[name]["lengths"], lib, tmp_path, chunks=1).length_figure_data()
    with pytest.raises(ValueError):
        mask_of([500, 0, 700], lib, tmp_path, chunks=1).length_figure_data()
    empty = sdust.LqMaskMI355X(str(tmp_path), lib=lib)
    with pytest.raises(ValueError):
        empty.length_figure_data()


def test_emulated_length_figure(emu_lib, tmp_path):
    check_length_figure(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_length_figure(gpu_lib, tmp_path):
    check_length_figure(gpu_lib, tmp_path)

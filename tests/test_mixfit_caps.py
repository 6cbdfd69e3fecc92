"""The mixture fits past their launch cap (LQ_MIX_MAX_BLOCKS fits a round, one block each; the others go round again), as
tests/test_launch_caps.py does for the chunk kernels: more two-value segments than one launch's grid holds -- with the grid shrunk by
LQMIX_TEST_MAX_BLOCKS and with the real cap and 100 more -- every one distinct, so that a fit written to another's place shows; and a
batch whose last segment is the only full-size one."""
import numpy as np
import pytest

from longqc_amd import mixfit as M
from tests import test_launch_caps as LC

CAP = LC.header_define("LQ_MIX_MAX_BLOCKS")
MAX_N = LC.header_define("LQ_MIX_MAX_N")


def pairs(count):
    lo = 1.0 + 0.125 * np.arange(count)
    return [np.array([a + 5.0, a]) for a in lo.tolist()], lo


def assert_pairs(fits, lo):
    """a segment {a, a + 5}: the split is between the two, each component keeps its value and reg_covar as its variance"""
    assert fits.shape == lo.shape and (fits["n"] == 2).all() and (fits["exit"] == M.EXIT_TOL).all() and (fits["n_iter"] >= 1).all()
    assert np.allclose(fits["mu"][:, 0], lo, rtol=1e-12, atol=0) and np.allclose(fits["mu"][:, 1], lo + 5.0, rtol=1e-12, atol=0)
    assert np.allclose(fits["w"], 0.5, rtol=1e-12, atol=0) and np.allclose(fits["s"], 1e-6, rtol=1e-6, atol=0)


def check_shrunk_grid(lib, monkeypatch):
    segs, lo = pairs(23)
    monkeypatch.delenv("LQMIX_TEST_MAX_BLOCKS", raising=False)
    whole = M.gmm2_raw(segs, lib=lib)
    monkeypatch.setenv("LQMIX_TEST_MAX_BLOCKS", "4")              # six rounds, the last one partial
    shrunk = M.gmm2_raw(segs, lib=lib)
    assert_pairs(whole, lo)
    assert shrunk.tobytes() == whole.tobytes()
    start = [(3.0, 2.0, 1.0, 1.0)] * len(segs)
    shrunk_l = M.lognorm_norm_raw(segs, start, max_iter=3, lib=lib)
    monkeypatch.delenv("LQMIX_TEST_MAX_BLOCKS")
    assert shrunk_l.tobytes() == M.lognorm_norm_raw(segs, start, max_iter=3, lib=lib).tobytes()
    assert (shrunk_l["n_iter"] == 4).all() and len({r.tobytes() for r in shrunk_l}) == len(segs)


def check_past_the_real_cap(lib, monkeypatch):
    monkeypatch.delenv("LQMIX_TEST_MAX_BLOCKS", raising=False)
    count = CAP + 100
    LC.assert_past_cap("k_mix_gmm2, fits", count, CAP, CAP)
    segs, lo = pairs(count)
    fits = M.gmm2_raw(segs, lib=lib)
    assert_pairs(fits, lo)
    for k in (0, CAP - 1, CAP, count - 1):
        assert fits[k].tobytes() == M.gmm2_raw([segs[k]], lib=lib)[0].tobytes()


def check_full_size_last(lib):
    rng = np.random.default_rng(12)
    big = np.round(np.concatenate([rng.uniform(0.5, 80, MAX_N // 5), rng.normal(28, 3, MAX_N - MAX_N // 5)]), 3)
    segs, lo = pairs(5)
    fits = M.gmm2_raw(segs + [big], max_iter=4, lib=lib)
    assert_pairs(fits[:5], lo)
    assert fits[5]["n"] == MAX_N and fits[5].tobytes() == M.gmm2_raw([big], max_iter=4, lib=lib)[0].tobytes()
    start = [(3.0, 2.0, 1.0, 1.0)] * 5 + [(40.0, 25.0, 3.3, 1.0)]
    logn = M.lognorm_norm_raw(segs + [big + 1.0], start, max_iter=2, lib=lib)
    assert logn[5]["n"] == MAX_N and logn[5].tobytes() == M.lognorm_norm_raw([big + 1.0], start[5:], max_iter=2, lib=lib)[0].tobytes()


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_fits_past_a_shrunk_grid(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_shrunk_grid(emu_lib, monkeypatch)


def test_emulated_fits_past_the_real_cap(emu_lib, monkeypatch):
    check_past_the_real_cap(emu_lib, monkeypatch)


def test_emulated_full_size_segment_last(emu_lib):
    check_full_size_last(emu_lib)


@pytest.mark.gpu
def test_gpu_fits_past_the_caps(gpu_lib, monkeypatch):
    check_shrunk_grid(gpu_lib, monkeypatch)
    check_past_the_real_cap(gpu_lib, monkeypatch)
    check_full_size_last(gpu_lib)

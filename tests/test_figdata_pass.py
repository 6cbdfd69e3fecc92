"""The figure data end to end: SampleQCPass.run_file on tests/golden/tiny_all.fq.gz with the device draw, then figures()
(LqGCMI355X.figure_data, LqMaskMI355X.length_figure_data over longqc_amd/figdata.py), under the wave emulator and on the GPU:

  * the three histograms are bit-equal to np.histogram(..., density=True) on gc.r_frac, gc.c_frac and the lengths of the table's third
    column, with the reference's edges np.arange(min, max + b_width, b_width);
  * the KDE curves are figdata.gaussian_kde_curve's called directly on the same arrays (the same bytes), the bandwidths scott_bandwidth's,
    and where scipy is importable both curves lie within tol + (12 / h + n) 2^-53 of scipy.stats.gaussian_kde -- tol the first-order
    bound of test_figdata_kde.py, computed here from the terms;
  * json_block(with_gamma=True) has the keys of longQC.py:495-502 in their order and the fit of length_figure_data(); json_block() is what
    it was, byte for byte as JSON;
  * a pass of one read has no read KDE and no length fit, a pass of one short read (one window at most) and a pass whose reads are all
    shorter than 750 bases (no window drawn, c_frac empty) raise the documented ValueErrors from figure_data(); gc_stats() goes on working."""
import json
import math
import os

import numpy as np
import pytest

from longqc_amd import chunkpass
from longqc_amd import figdata as F
from tests import test_figdata_kde as TK
from tests.conftest import GOLDEN
from tests.test_sdust_table import ADP3, ADP5

EPS = 2.0 ** -53


def scipy_check(x, xs, curve, h):
    try:
        from scipy.stats import gaussian_kde
    except ImportError:
        return None
    want = gaussian_kde(x)(xs)
    near = np.flatnonzero(want >= 1e-6 * want.max())
    tol = TK.first_order_tol(x, xs, h)[near]
    r = np.abs(curve[near] - want[near]) / want[near] / (tol + (12 / h + x.shape[0]) * EPS)
    assert (r <= 1).all(), (near[r > 1], curve[near][r > 1], want[near][r > 1])
    return float(r.max())


def check_figures(lib, tmp_path):
    path = os.path.join(GOLDEN, "tiny_all.fq.gz")
    p = chunkpass.SampleQCPass(str(tmp_path / "run"), "ont-ligation", adp5=ADP5, adp3=ADP3, nsample=15, gc_draw="device", gc_seed=3, lib=lib)
    try:
        assert len(p.run_file(path, chunk_size=100000, str_overhead=49)) >= 3
        before = json.dumps(p.mask.json_block())
        fig = p.figures()
        assert set(fig) == {"gc", "length"}
        gc, ln = fig["gc"], fig["length"]
        assert set(gc) == {"xs", "read_hist", "chunk_hist", "read_kde", "chunk_kde", "read_bandwidth", "chunk_bandwidth", "mean", "sd"}
        assert set(ln) == {"hist", "gamma_params", "mean_length", "n50", "longest"}
        assert gc["xs"].tobytes() == np.linspace(0, 1.0, 50).tobytes()
        assert [gc["mean"], gc["sd"]] == p.gc.gc_stats()
        for key, frac in (("read", p.gc.r_frac), ("chunk", p.gc.c_frac)):
            x = np.array(frac, dtype=np.float32)
            assert x.shape[0] > 100
            edges = np.arange(min(frac), max(frac) + 0.02, 0.02)    # lq_gcfrac.py:58,63
            want, _ = np.histogram(frac, bins=edges, density=True)
            e, c, d = gc[key + "_hist"]
            assert e.tobytes() == edges.tobytes() and d.tobytes() == want.tobytes() and c.tolist() == np.histogram(frac, bins=edges)[0].tolist()
            curve, h = F.gaussian_kde_curve(x, gc["xs"], lib=lib, return_bandwidth=True)
            assert gc[key + "_kde"].tobytes() == curve.tobytes() and gc[key + "_bandwidth"] == h == F.scott_bandwidth(x)
            r = scipy_check(x, gc["xs"], gc[key + "_kde"], h)
            print("%s: %d values, h %r, against scipy %s of the bound" % (key, x.shape[0], h, "not compared" if r is None else "%.4f" % r))
        p.mask.close_pool()
        lens = np.array([int(row.split("\t")[2]) for row in open(p.mask.get_outfile_path()).read().splitlines()])
        assert lens.shape[0] == 120
        edges = np.arange(min(lens), max(lens) + 1000, 1000)        # lq_gamma.py:54
        want, _ = np.histogram(lens, bins=edges, density=True)
        assert ln["hist"][0].tobytes() == edges.tobytes() and ln["hist"][2].tobytes() == want.tobytes()
        s = p.summary()
        assert (ln["mean_length"], ln["n50"], ln["longest"]) == (s["mean_length"], s["n50"], s["longest"])
        a, scale = ln["gamma_params"]
        mean, mean_log = lens.mean(), math.fsum(math.log(v) for v in lens.tolist()) / lens.shape[0]
        assert abs(math.log(a) - F.digamma(a) - (math.log(mean) - mean_log)) < 1e-12 and abs(a * scale - mean) < 1e-9 * mean
        try:
            from scipy.stats import gamma
            sa, _, sscale = gamma.fit(lens, floc=0)
            assert abs(a - sa) <= 1e-9 * sa and abs(scale - sscale) <= 1e-9 * sscale
        except ImportError:
            pass
        with_gamma = p.mask.json_block(with_gamma=True)
        assert list(with_gamma) == ["Yield", "Q7 bases", "Longest_read", "Num_of_reads", "Length_stats"]
        assert list(with_gamma["Length_stats"]) == ["gamma_params", "Mean_read_length", "N50_read_length"]      # longQC.py:500-502
        assert with_gamma["Length_stats"]["gamma_params"] == [a, scale]
        stripped = json.loads(json.dumps(with_gamma))
        del stripped["Length_stats"]["gamma_params"]
        assert json.dumps(stripped) == before == json.dumps(p.mask.json_block()) == json.dumps(p.mask.json_block(with_gamma=False))
    finally:
        p.close()


def reads_of(lens, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [["r%d" % i, acgt[rng.integers(0, 4, l)].tobytes().decode(), "5" * l] for i, l in enumerate(lens)]


def check_degenerate_passes(lib, tmp_path):
    def a_pass(tag, lens):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "ont-ligation", nsample=5, gc_draw="device", gc_seed=1, lib=lib)
        p.add_chunk(reads_of(lens, 7))
        return p
    p = a_pass("one", [9000])                                       # one read: windows, but no read KDE and no spread of lengths
    try:
        gc = p.gc.figure_data()
        assert gc["read_kde"] is None and gc["read_bandwidth"] is None and gc["chunk_kde"].shape == (50,) and len(p.gc.c_frac) > 1
        assert gc["read_hist"][1].sum() <= 1                        # (np.arange(min, min + 0.02, 0.02): one edge, or two and the read between them)
        with pytest.raises(ValueError):
            p.mask.length_figure_data()
        with pytest.raises(ValueError):
            p.figures()
        assert "gamma_params" not in p.mask.json_block()["Length_stats"]
    finally:
        p.close()
    p = a_pass("one_short", [800])                                  # int(800 / 150 * 0.2) = 1 draw: one window or none, no chunk KDE
    try:
        assert len(p.gc.r_frac) == 1 and len(p.gc.c_frac) <= 1
        with pytest.raises(ValueError):
            p.gc.figure_data()
        assert p.gc.gc_stats()[1] == 0
    finally:
        p.close()
    p = a_pass("short", [700, 749, 300, 12, 500])                   # int(l / 150 * 0.2) = 0 draws for l < 750: c_frac stays empty
    try:
        assert len(p.gc.r_frac) == 5 and len(p.gc.c_frac) == 0
        with pytest.raises(ValueError):
            p.gc.figure_data()
        mean, sd = p.gc.gc_stats()
        assert 0.3 < mean < 0.7 and sd > 0
        assert p.mask.length_figure_data()["hist"][1].tolist() == [5]          # (the lengths have a figure of their own)
    finally:
        p.close()


def test_emulated_figures_of_a_pass(emu_lib, tmp_path):
    check_figures(emu_lib, tmp_path)


def test_emulated_degenerate_passes(emu_lib, tmp_path):
    check_degenerate_passes(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_figures_of_a_pass(gpu_lib, tmp_path):
    check_figures(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_degenerate_passes(gpu_lib, tmp_path):
    check_degenerate_passes(gpu_lib, tmp_path)

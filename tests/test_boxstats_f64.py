"""lqfig_boxstats_f64 (kernels_boxstats_f64.hpp, longqc_amd.rs.box_stats_f64) against matplotlib.cbook.boxplot_stats, double for double,
under the wave emulator and on the GPU:

  * on the golden groups: ReadScore by np.floor((HQRegionEnd - HQRegionStart) / 1000) of every run of tests/golden/rs.json, whose boxes
    make_rs_golden.py recorded from matplotlib itself;
  * on random groups of 1, 2, 3, 4, 5 and 1 000 values with negative values, -0.0 and +0.0 and repeated values, against
    tests/test_boxstats.py's box_of, which is matplotlib's box (checked there against matplotlib and the golden file).  Doubles are
    compared with ==, under which -0.0 equals +0.0, as numpy's own sort treats them;
  * the layout of sorted[] and the boxes' places; the refusals;
  * and the thousandths entry lqfig_boxstats still gives what it gave on tests/golden/boxstats.json."""
import functools
import json
import os

import numpy as np
import pytest

from longqc_amd import api, rs
from tests import test_boxstats as TB
from tests.conftest import GOLDEN

GOLD = json.load(open(os.path.join(GOLDEN, "rs.json")))
STATS = ("q1", "med", "q3", "whislo", "whishi", "median")


def oracle(key, x, interval=0.0, whis=1.5):
    g = TB.groups_of(key, interval)
    out = []
    for gid in np.unique(g).tolist():
        v = np.asarray(x, dtype=np.float64)[g == gid]
        out.append(dict(TB.box_of(v, whis), group=int(gid), n=int(v.size)))
    return out


def same(got, want, what):
    assert got["group"].tolist() == [b["group"] for b in want] and got["n"].tolist() == [b["n"] for b in want], what
    for k in STATS:
        assert got[k].tolist() == [b[k] for b in want], (what, k)
    for f, b in zip(got["fliers"], want):
        assert f.dtype == np.float64 and sorted(f.tolist()) == sorted(b["fliers"]), (what, b["group"])


@functools.lru_cache(maxsize=None)
def random_groups():
    """-> (key, x, the oracle's boxes): groups 10, 20, .. of 1, 2, 3, 4, 5, 1000 and again 1 .. 5 values; computed once, nobody changes them"""
    rng = np.random.default_rng(21)
    key, x = [], []
    for gid, n in enumerate((1, 2, 3, 4, 5, 1000, 1, 2, 3, 4, 5)):
        if gid < 6:
            v = rng.normal(0.0, 3.0, n)                                 # negative and positive
            v[rng.integers(0, n, n // 5)] = rng.choice(v, n // 5)       # repeated values
        else:
            v = rng.choice(np.array([-0.0, 0.0, -1.5, 2.25, 0.0, -0.0]), n)
        key += [10 * (gid + 1)] * n
        x += v.tolist()
    x[5 + 17], x[5 + 18], x[5 + 400], x[5 + 401] = -0.0, 0.0, 1e-300, -1e300
    order = rng.permutation(len(key))
    key, x = np.array(key, np.uint32)[order], np.array(x)[order]
    key.setflags(write=False); x.setflags(write=False)
    return key, x, oracle(key, x)


def check_golden_groups(lib):
    for run, want in GOLD["runs"].items():
        c = {k: np.array(v["values"], dtype=v["dtype"]) for k, v in want["columns"].items()}
        key, x = (c["HQRegionEnd"] - c["HQRegionStart"]).astype(np.uint32), c["ReadScore"].astype(np.float64)
        got = rs.box_stats_f64(key, x, 1000.0, lib=lib)
        same(got, want["box"], run)


def check_random_groups(lib):
    key, x, want = random_groups()
    assert (x < 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    same(rs.box_stats_f64(key, x, lib=lib), want, "random groups")
    for whis in (0.0, 3.0):
        same(rs.box_stats_f64(key, x, 0.0, whis, lib=lib), oracle(key, x, 0.0, whis), "whis %r" % whis)
    same(rs.box_stats_f64(key, x, 25.0, lib=lib), oracle(key, x, 25.0), "interval 25")      # 10 and 20 share group 0, 30 and 40 group 1, ...
    s, b = rs.box_stats_f64_raw(key, x, lib=lib)
    order = np.lexsort((x, key))
    assert np.array_equal(s, x[order])                                  # group by group, ascending inside
    zeros = np.flatnonzero((s[:-1] == 0) & (s[1:] == 0) & (key[order][:-1] == key[order][1:]))
    assert zeros.size and not (np.signbit(s[zeros + 1]) & ~np.signbit(s[zeros])).any()      # -0.0 never behind +0.0
    firsts = np.concatenate([[0], np.flatnonzero(np.diff(key[order])) + 1])
    assert b["first"].tolist() == firsts.tolist() and (b["n"] == b["n_all"]).all() and int(b["n"].sum()) == x.size and (b["reserved"] == 0).all()
    for r in b:
        st = s[int(r["first"]):int(r["first"] + r["n"])]
        assert (r["mid_lo"], r["mid_hi"]) == (st[(st.size - 1) // 2], st[st.size // 2])


def check_refusals(lib):
    empty_s, empty_b = rs.box_stats_f64_raw(np.zeros(0, np.uint32), np.zeros(0), lib=lib)
    assert empty_s.size == 0 and empty_b.size == 0
    for x, interval, whis, code in (([1.0, float("nan")], 0.0, 1.5, -5), ([1.0, 2.0], -1.0, 1.5, -1), ([1.0, 2.0], 0.0, float("inf"), -1),
                                    ([1.0, 2.0], 1e-9, 1.5, -5)):
        with pytest.raises(api.LqcovError) as e:
            rs.box_stats_f64([7, 4000000000], x, interval, whis, lib=lib)
        assert e.value.code == code, (x, interval, whis, str(e.value))


def check_all(lib):
    check_golden_groups(lib)
    check_random_groups(lib)
    check_refusals(lib)
    TB.check_golden_cases(lib)                                          # the thousandths entry is what it was


def test_emulated_f64_boxes_are_matplotlibs(emu_lib):
    check_all(emu_lib)


def test_emulated_f64_boxes_do_not_depend_on_the_grid(emu_lib, monkeypatch):
    for blocks in ("1", "3"):
        monkeypatch.setenv("LQBOX_TEST_MAX_BLOCKS", blocks)
        check_golden_groups(emu_lib)
        check_random_groups(emu_lib)


@pytest.mark.gpu
def test_gpu_f64_boxes_are_matplotlibs(gpu_lib):
    check_all(gpu_lib)

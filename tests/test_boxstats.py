"""Box-plot statistics by group (k_box_* of kernels_boxstats.hpp behind lqfig_boxstats; figdata.box_stats, figdata.box_stats_raw) under the
wave emulator and on the GPU.  Every double and every group's sorted fliers are compared for exact equality (==, so -0.0 is 0.0) with

  * `oracle`, a numpy restatement of matplotlib.cbook.boxplot_stats(x, whis) on each group's non-missing values and of np.median, which
  * is itself compared with matplotlib and pandas where they import, and on every machine with tests/golden/boxstats.json, written by
    tests/golden/make_boxstats_golden.py from matplotlib 3.10.8 / pandas 2.3.3.

Which case notices which slip:
  a + (b - a) t for every t            the pairs (n = 2: t = 0.25 and 0.75); built once, below: test_a_one_sided_interpolation_is_noticed picks,
                                       with numpy, pairs on which the two formulas differ, and asserts that they do
  a fused multiply-add                 the same pairs and the random groups: a + d t rounded once differs where the product is inexact
  the reciprocal for the length bin    "length bins": every length 0 .. 30000 by 49; the test asserts from numpy that such lengths change bin
  the percentile's value as the median "pairs" in the golden file: (a + b) / 2 against a + (b - a) 0.5 -- the two are compared as they come
  whiskers that ignore the fallback    [0, 0, 0, 100.000] and its mirror
  missing values sorted first / kept   "missing values"
  a sort over too few key bits         group ids {0, 1, 300, 70000, 2^31}
  a second round of a launch lost      "past the launch cap" (elements) and "more groups than a launch holds" (groups)"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from longqc_amd import api
from longqc_amd import figdata as F
from tests import test_launch_caps as LC
from tests.conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "longqc_amd", "csrc")
MISSING = F.MISSING
GOLD = json.load(open(os.path.join(GOLDEN, "boxstats.json")))
STATS = ("q1", "med", "q3", "whislo", "whishi", "median")


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def percentile_linear(x, q):
    """np.percentile(x, 100 q) for ascending doubles, method "linear": every operation on np.float64 scalars, rounded on its own"""
    n = x.shape[0]
    vi = np.float64(n - 1) * np.float64(q)
    lo = int(np.floor(vi))
    t = vi - np.float64(lo)
    a, b = x[lo], x[min(lo + 1, n - 1)]
    d = b - a
    return b - d * (np.float64(1) - t) if t >= 0.5 else a + d * t


def box_of(x, whis=1.5):
    """matplotlib.cbook.boxplot_stats(x, whis)[0] without mean and notch, and np.median, for the doubles x (no NaN, at least one)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.shape[0]
    q1, med, q3 = (percentile_linear(x, q) for q in (0.25, 0.5, 0.75))
    iqr = q3 - q1
    hi = x[x <= q3 + np.float64(whis) * iqr]
    whishi = q3 if hi.shape[0] == 0 or hi.max() < q3 else hi.max()
    lo = x[x >= q1 - np.float64(whis) * iqr]
    whislo = q1 if lo.shape[0] == 0 or lo.min() > q1 else lo.min()
    return {"q1": float(q1), "med": float(med), "q3": float(q3), "whislo": float(whislo), "whishi": float(whishi),
            "median": float((x[(n - 1) // 2] + x[n // 2]) / 2), "fliers": np.concatenate([x[x < whislo], x[x > whishi]]).tolist()}


def groups_of(key, interval):
    key = np.asarray(key, dtype=np.int64)
    return np.floor(key / interval).astype(np.int64) if interval else key


@functools.lru_cache(maxsize=None)
def oracle_of(make, *args):
    """the inputs a case builder gives and their boxes, computed once for every test of the session; nobody changes them"""
    key, thou = make(*args)
    key.setflags(write=False); thou.setflags(write=False)
    return key, thou, oracle(key, thou, *args)


def oracle(key, thou, interval=0.0, whis=1.5):
    """-> the boxes in the golden file's form: one dict per group that occurs, ascending"""
    thou = np.asarray(thou, dtype=np.int64)
    g = groups_of(key, interval)
    order = np.argsort(g, kind="stable")
    gs, ts = g[order], thou[order]
    cuts = np.flatnonzero(np.diff(gs)) + 1
    out = []
    for gid, t in zip(gs[np.concatenate([[0], cuts]).astype(np.int64)].tolist() if gs.shape[0] else [], np.split(ts, cuts)):
        x = t[t != MISSING] / 1000
        b = {"group": gid, "n_all": int(t.shape[0]), "n": int(x.shape[0])}
        b.update(box_of(x, whis) if x.shape[0] else dict({k: None for k in STATS}, fliers=[]))
        out.append(b)
    return out


def same_boxes(got, want, what):
    """got: figdata.box_stats' dict; want: boxes in the golden file's form"""
    assert got["group"].tolist() == [b["group"] for b in want], what
    assert got["n_all"].tolist() == [b["n_all"] for b in want] and got["n"].tolist() == [b["n"] for b in want], what
    for k in STATS:
        for j, b in enumerate(want):
            g = float(got[k][j])
            assert (np.isnan(g) if b[k] is None else g == b[k]), (what, k, b["group"], g, b[k])
    assert len(got["fliers"]) == len(want)
    for f, b in zip(got["fliers"], want):
        assert f.dtype == np.float64 and sorted(f.tolist()) == sorted(b["fliers"]), (what, b["group"], f, b["fliers"])


def check_raw(key, thou, interval, s, b, what):
    """the layout lqfig_boxstats promises: sorted[] group by group, values ascending and the missing ones last; the boxes' places"""
    g = groups_of(key, interval)
    thou = np.asarray(thou, dtype=np.int64)
    rank = np.where(thou == MISSING, np.int64(2) ** 40, thou)
    order = np.lexsort((rank, g))
    assert s.tolist() == thou[order].tolist(), what
    firsts = np.concatenate([[0], np.flatnonzero(np.diff(g[order])) + 1]) if g.shape[0] else np.zeros(0, np.int64)
    assert b["first"].tolist() == firsts.tolist() and int(b["n_all"].sum()) == g.shape[0], what
    assert (b["reserved"] == 0).all()
    for r in b:
        st = s[int(r["first"]):int(r["first"] + r["n_all"])]
        assert int((st != MISSING).sum()) == int(r["n"]), what
        if r["n"]:
            assert (r["mid_lo"], r["mid_hi"]) == (st[(int(r["n"]) - 1) // 2], st[int(r["n"]) // 2]), what
        else:
            assert r["mid_lo"] == r["mid_hi"] == MISSING and r["n_low"] == r["n_high"] == 0, what


def run_case(lib, key, thou, interval, whis, want, what):
    same_boxes(F.box_stats(key, thou, interval, whis, lib=lib), want, what)
    s, b = F.box_stats_raw(key, thou, interval, whis, lib=lib)
    check_raw(key, thou, interval, s, b, what)
    return s, b


# ---- the oracle against matplotlib, pandas and the golden file -----------------------------------------------------------
def test_the_oracle_gives_the_golden_files_numbers():
    assert GOLD["missing"] == MISSING
    for c in GOLD["cases"]:
        got = oracle(c["key"], c["thou"], c["interval"], c["whis"])
        for g, w in zip(got, c["boxes"]):
            assert g == dict(w, fliers=sorted(w["fliers"])), (c["name"], g, w)
        assert len(got) == len(c["boxes"])


def test_the_oracle_is_matplotlibs_and_pandas():
    cbook = pytest.importorskip("matplotlib.cbook")
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(3)
    for trial in range(300):
        n = int(rng.integers(1, 14))
        x = rng.integers(-2000, 40000, n) / 1000 if trial % 3 else rng.integers(0, 6, n) * 1.5
        whis = (1.5, 0.0, 0.7)[trial % 3]
        st, mine = cbook.boxplot_stats(x, whis=whis)[0], box_of(x, whis)
        for k in ("q1", "med", "q3", "whislo", "whishi"):
            assert float(st[k]) == mine[k], (x, k)
        assert sorted(st["fliers"].tolist()) == mine["fliers"]
        assert mine["median"] == float(np.median(x)) == float(pd.Series(x).median())
    key, thou = rng.integers(0, 9, 400), rng.integers(0, 30000, 400)
    med = pd.DataFrame({"g": key, "v": thou / 1000}).groupby("g")["v"].median()
    assert [b["median"] for b in oracle(key, thou)] == med.tolist()


def test_the_golden_file_holds_what_the_issue_names():
    names = " | ".join(c["name"] for c in GOLD["cases"])
    for part in ("sizes 1 2 3 4 5 8 9", "pairs", "ties and all equal", "falls back", "far outlier", "negative", "missing", "every key byte", "interval 49.0"):
        assert part in names
    by = {c["name"]: c for c in GOLD["cases"]}
    b = by["the whisker falls back to the quartile"]["boxes"]
    assert (b[0]["whishi"], b[0]["q3"], b[0]["fliers"]) == (25.0, 25.0, [100.0]) and (b[1]["whislo"], b[1]["q1"], b[1]["fliers"]) == (75.0, 75.0, [0.0])
    assert [x["n"] for x in by["missing values"]["boxes"]] == [0, 3, 0, 1, 3]
    assert [x["group"] for x in by["group ids in every key byte"]["boxes"]] == [0, 1, 300, 70000, 2 ** 31]
    assert any(x["median"] != x["med"] for c in GOLD["cases"] for x in c["boxes"] if x["n"])      # (the two medians are not one rule)
    eq = by["ties and all equal"]["boxes"][1]
    assert eq["q1"] == eq["q3"] == eq["whislo"] == eq["whishi"] == 3.0 and eq["fliers"] == []


# ---- the cases the test makes itself ------------------------------------------------------------------------------------
def one_sided(a, b, t):
    return a + (b - a) * np.float64(t)


def pairs_where_the_formulas_differ(count=24):
    """pairs of thousandths (a < b) on which numpy's two-sided rule and a + (b - a) t give another q3 (t = 0.75 at n = 2)"""
    rng = np.random.default_rng(8)
    out = []
    while len(out) < count:
        a, b = sorted(rng.integers(0, 60000, 2).tolist())
        x = np.array([a, b]) / 1000
        if a != b and percentile_linear(x, 0.75) != one_sided(x[0], x[1], 0.75):
            out.append((a, b))
    return out


def length_bins(interval):
    """lengths 0 .. 30000 (every one for 49, the interval whose reciprocal misplaces some; every 7th otherwise) with a QV each"""
    lens = np.arange(0, 30001) if interval == 49 else np.arange(0, 30001, 7)
    rng = np.random.default_rng(int(interval))
    lens = np.concatenate([lens, rng.integers(0, 30001, 500)])
    return rng.permutation(lens).astype(np.uint32), rng.integers(0, 45000, lens.shape[0]).astype(np.int32)


def past_the_cap():
    cap, block = LC.header_define("LQ_BOX_MAX_BLOCKS"), LC.header_define("LQ_BOX_THREADS")
    n = cap * block + 300
    LC.assert_past_cap("k_box_keys / k_box_flags / k_box_heads, elements", n, cap * block, block)
    assert n <= 20000 + cap * block
    rng = np.random.default_rng(5)
    key = rng.integers(0, 3, n).astype(np.uint32) * 1000
    key[-250:] = 2000                                                # (the second round has all three groups' members)
    thou = rng.integers(-5000, 60000, n).astype(np.int32)
    thou[rng.integers(0, n, 40)] = MISSING
    return key, thou


def many_groups():
    cap, block = LC.header_define("LQ_BOX_MAX_BLOCKS"), LC.header_define("LQ_BOX_THREADS")
    n_groups = cap * block + 130
    LC.assert_past_cap("k_box_stats, groups", n_groups, cap * block, block)
    rng = np.random.default_rng(6)
    key = np.concatenate([np.arange(n_groups) * 3, rng.integers(0, n_groups, 900) * 3]).astype(np.uint32)      # (gaps; some groups of two or more)
    return rng.permutation(key).astype(np.uint32), rng.integers(0, 30000, key.shape[0]).astype(np.int32)


def check_golden_cases(lib):
    for c in GOLD["cases"]:
        run_case(lib, c["key"], c["thou"], c["interval"], c["whis"], c["boxes"], c["name"])


def check_pairs(lib):
    pairs = pairs_where_the_formulas_differ()
    key = np.repeat(np.arange(len(pairs)), 2)
    thou = np.array(pairs).ravel()
    run_case(lib, key, thou, 0.0, 1.5, oracle(key, thou), "pairs on which the one-sided formula differs")


def check_length_bins(lib):
    for interval in (3000.0, 1234.5, 7.0, 49.0):
        lens, qv, want = oracle_of(length_bins, interval)
        by_division, by_reciprocal = np.floor(lens / interval), np.floor(lens * (1 / interval))
        if interval == 49.0:                                            # (of the four, 49 alone has such lengths below 30001: 315 of them)
            assert (by_division != by_reciprocal).sum() >= 100          # a reciprocal slip moves these reads into another bin
        run_case(lib, lens, qv, interval, 1.5, want, "length bins, interval %r" % interval)


def check_caps(lib):
    key, thou, want = oracle_of(past_the_cap)
    s, b = run_case(lib, key, thou, 0.0, 1.5, want, "past the launch cap")
    assert b["group"].tolist() == [0, 1000, 2000]
    key, thou, want = oracle_of(many_groups)
    assert len(want) > LC.header_define("LQ_BOX_MAX_BLOCKS") * LC.header_define("LQ_BOX_THREADS")
    run_case(lib, key, thou, 0.0, 1.5, want, "more groups than a launch holds")


def check_whis_and_empty(lib):
    rng = np.random.default_rng(12)
    key, thou = rng.integers(0, 5, 300), rng.integers(0, 30000, 300)
    for whis in (0.0, 0.7, 3.0):
        run_case(lib, key, thou, 0.0, whis, oracle(key, thou, 0.0, whis), "whis %r" % whis)
    got = F.box_stats(np.zeros(0, np.uint32), np.zeros(0, np.int32), lib=lib)
    assert all(got[k].shape == (0,) for k in ("group", "n", "q1", "median")) and got["fliers"] == []
    s, b = F.box_stats_raw([], [], lib=lib)
    assert s.shape == (0,) and b.shape == (0,)


def check_box_cap_and_bytes(lib):
    c = next(c for c in GOLD["cases"] if c["name"] == "missing values")
    groups = len(c["boxes"])
    key, thou = np.array(c["key"], dtype=np.uint32), np.array(c["thou"], dtype=np.int32)
    out, boxes, nb, err = np.zeros(key.size, np.int32), np.zeros(groups, dtype=F.BOX), C.c_uint32(77), C.create_string_buffer(512)
    call = lambda cap: F._box_lib(lib).lqfig_boxstats(0, key.ctypes.data, thou.ctypes.data, key.size, 0.0, 1.5, out.ctypes.data, boxes.ctypes.data, cap, C.byref(nb), err, 512)
    assert call(groups - 1) == -1 and nb.value == groups and b"box_cap" in err.value          # LQCOV_E_ARG, the number still written
    assert not boxes["n_all"].any()
    assert call(groups) == 0 and nb.value == groups                                          # the retry
    s1, b1 = F.box_stats_raw(key, thou, lib=lib)
    assert boxes.tobytes() == b1.tobytes() and out.tobytes() == s1.tobytes()
    with pytest.raises(api.LqcovError) as e:
        F.box_stats_raw(key, thou, lib=lib, box_cap=1)
    assert e.value.code == -1
    key, thou = many_groups()                                         # identical bytes from two calls, at a size with several tiles and passes
    s1, b1 = F.box_stats_raw(key, thou, lib=lib)
    s2, b2 = F.box_stats_raw(key, thou, lib=lib)
    assert s1.tobytes() == s2.tobytes() and b1.tobytes() == b2.tobytes()


def check_refusals(lib):
    key, thou = np.array([1, 2], np.uint32), np.array([5, 6], np.int32)
    for kw in ({"interval": -1.0}, {"interval": np.inf}, {"interval": np.nan}, {"whis": -0.5}, {"whis": np.inf}, {"whis": np.nan}):
        with pytest.raises(api.LqcovError) as e:
            F.box_stats(key, thou, lib=lib, **kw)
        assert e.value.code == -1, kw                               # LQCOV_E_ARG
    with pytest.raises(api.LqcovError) as e:
        F.box_stats(key, np.array([5, 2 ** 31 - 1], np.int32), lib=lib)
    assert e.value.code == -5                                       # LQCOV_E_DOMAIN: the value whose key is the missing one's
    with pytest.raises(api.LqcovError) as e:
        F.box_stats(np.array([1, 2 ** 32 - 1], np.uint32), thou, interval=0.5, lib=lib)
    assert e.value.code == -5                                       # a group of 2^32 or more
    nb, err = C.c_uint32(5), C.create_string_buffer(512)
    assert F._box_lib(lib).lqfig_boxstats(0, None, None, 2 ** 32, 0.0, 1.5, None, None, 0, C.byref(nb), err, 512) == -5 and nb.value == 0
    assert F.box_stats(key, thou, lib=lib)["group"].tolist() == [1, 2]      # the next call works
    with pytest.raises(ValueError):
        F.box_stats(key, thou[:1], lib=lib)
    with pytest.raises(TypeError):
        F.box_stats(key, np.array([0.5, 1.0]), lib=lib)
    with pytest.raises(ValueError):
        F.box_stats(np.array([-1, 2]), thou, lib=lib)


def check_all(lib):
    check_golden_cases(lib)
    check_pairs(lib)
    check_length_bins(lib)
    check_caps(lib)
    check_whis_and_empty(lib)
    check_box_cap_and_bytes(lib)
    check_refusals(lib)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_boxes_are_matplotlibs(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_all(emu_lib)


def test_emulated_boxes_do_not_depend_on_the_grid(emu_lib, monkeypatch):
    key, thou = past_the_cap()
    s1, b1 = F.box_stats_raw(key[:3000], thou[:3000], lib=emu_lib)
    monkeypatch.setenv("LQBOX_TEST_MAX_BLOCKS", "2")
    s2, b2 = F.box_stats_raw(key[:3000], thou[:3000], lib=emu_lib)
    assert s1.tobytes() == s2.tobytes() and b1.tobytes() == b2.tobytes()


def variant(tmp_path, define):
    """boxstats.cpp built again for the emulator with a test-only define (the rest of the library comes from the session's build)"""
    so = str(tmp_path / ("liblqbox_%s.so" % define.split("=")[0].lower()))
    emu = os.path.join(ROOT, "tests", "emu")
    r = subprocess.run(["g++", "-DLQ_EMU", "-D" + define, "-include", os.path.join(emu, "hipemu.hpp"), "-O1", "-std=c++17", "-fPIC",
                        "-Wno-unknown-pragmas", "boxstats.cpp", "-shared", "-o", so, os.path.join(emu, "liblqcov_emu.so"), "-Wl,-rpath," + emu, "-lz"],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return C.CDLL(so)


def test_a_one_sided_interpolation_is_noticed(emu_lib, tmp_path):
    """LQ_BOX_LERP_TWO_SIDED=0 takes a + (b - a) t for every t: the n = 2 pairs fail (their q3, t = 0.75), the length bins do not care"""
    pairs = pairs_where_the_formulas_differ()
    for a, b in pairs:                                              # the two formulas do differ at thousandths
        x = np.array([a, b]) / 1000
        assert percentile_linear(x, 0.75) != one_sided(x[0], x[1], 0.75)
    lib = variant(tmp_path, "LQ_BOX_LERP_TWO_SIDED=0")
    key, thou = np.repeat(np.arange(len(pairs)), 2), np.array(pairs).ravel()
    got, want = F.box_stats(key, thou, lib=lib), oracle(key, thou)
    assert all(float(g) != w["q3"] for g, w in zip(got["q3"], want))
    assert [float(g) for g in got["q3"]] == [float(one_sided(a / np.float64(1000), b / np.float64(1000), 0.75)) for a, b in pairs]
    assert [float(g) for g in got["q1"]] == [w["q1"] for w in want]  # (t = 0.25: the same formula in both)
    with pytest.raises(AssertionError):
        check_pairs(lib)
    check_pairs(emu_lib)


def test_a_reciprocal_length_bin_is_noticed(emu_lib, tmp_path):
    """LQ_BOX_BIN_BY_DIVISION=0 takes floor(len * (1 / interval)): the length bins by 49 and 7 fail, groups without an interval do not"""
    lib = variant(tmp_path, "LQ_BOX_BIN_BY_DIVISION=0")
    with pytest.raises(AssertionError):
        check_length_bins(lib)
    assert F.box_stats([49], [1000], interval=49.0, lib=lib)["group"].tolist() == [0]
    assert F.box_stats([49], [1000], interval=49.0, lib=emu_lib)["group"].tolist() == [1]
    check_pairs(lib)


@pytest.mark.gpu
def test_gpu_boxes_are_matplotlibs(gpu_lib):
    check_all(gpu_lib)

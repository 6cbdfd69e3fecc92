"""The k_csv_* kernels and the f64 box kernels past their launch caps (kernels_csv.hpp, kernels_boxstats_f64.hpp), after the scheme of
tests/test_polread_caps.py: the smallest inputs that make every one of them run its grid-stride loop a second time, with partial last
units -- more bytes than one round of k_csv_marks, k_csv_rows and k_csv_starts takes, more (row, column) pairs than one round of
k_csv_parse, more rows than one round of k_csv_lengths and k_csv_pack (and so more masked rows than one round of k_pol_unkey and k_pol_nxx
as csv.cpp launches them); more elements than one round of k_boxd_keys, k_boxd_rekey and k_boxd_flags and more groups than one round of
k_boxd_stats.  Rows are as short as "1,2,3,.5".  Caps are read from the headers; the expected values come from numpy and from
tests/test_boxstats.py's box_of."""
import functools
import time

import numpy as np
import pytest

from longqc_amd import rs
from tests import test_boxstats as TB
from tests import test_launch_caps as LC


@functools.lru_cache(maxsize=None)
def table():
    """-> (the bytes, start, end, bases, score): computed once, nobody changes them"""
    cap, threads = LC.header_define("LQ_CSV_MAX_BLOCKS"), LC.header_define("LQ_CSV_THREADS")
    n = cap * threads + 100 * threads + 11                           # (four fifths of them under the mask: still more than a round)
    rng = np.random.default_rng(9)
    start = rng.integers(0, 10, n)
    end = start + rng.integers(0, 90, n)
    bases = end + rng.integers(1, 10, n)
    tenths = rng.integers(0, 10, n)                                     # the score: .0 to .9, every fifth row below or at the threshold
    text = "s,e,b,x\n" + "".join("%d,%d,%d,.%d\n" % r for r in zip(start.tolist(), end.tolist(), bases.tolist(), tenths.tolist()))
    score = np.array([float(".%d" % t) for t in range(10)])[tenths]
    for a in (start, end, bases, score):
        a.setflags(write=False)
    return text.encode(), start, end, bases, score


def check_table_past_cap(lib):
    cap, threads = LC.header_define("LQ_CSV_MAX_BLOCKS"), LC.header_define("LQ_CSV_THREADS")
    t0 = time.time()
    data, start, end, bases, score = table()
    n = start.size
    mask = score > 0.1
    LC.assert_past_cap("k_csv_marks / k_csv_rows / k_csv_starts, bytes", len(data), cap * threads, threads)
    LC.assert_past_cap("k_csv_parse, (row, column) pairs", 4 * n, cap * threads, threads)
    LC.assert_past_cap("k_csv_lengths / k_csv_pack, rows", n, cap * threads, threads)
    LC.assert_past_cap("k_pol_unkey / k_pol_nxx, masked rows", int(mask.sum()), cap * threads)
    assert int(mask.sum()) % threads != 0
    LC.timed("table input (%d rows, %d bytes)" % (n, len(data)), t0)
    t0 = time.time()
    with rs.StsTable(data, columns=(("x", rs.DOUBLE), ("s", rs.INT64), ("e", rs.INT64), ("b", rs.INT64)), lib=lib) as t:
        assert t.n_rows == n and t.stats["pieces"] == 1 and t.stats["fields_device"] == 4 * n and t.stats["fields_host"] == 0
        for name, want in (("s", start), ("e", end), ("b", bases)):
            LC.first_diff(t.column(name).tolist(), want.tolist(), cap * threads, "column " + name)
        assert np.array_equal(t.column("x").view(np.uint64), score.view(np.uint64))
        st = t.lengths("x", 0.1, "s", "e", "b")
        hq, nb = (end - start)[mask], bases[mask]
        desc = np.sort(hq)[::-1]
        cum = np.cumsum(desc)
        assert st == {"n": hq.size, "sum_hq": int(hq.sum()), "min_hq": int(hq.min()), "max_hq": int(hq.max()), "n50": int(desc[np.argmax(2 * cum >= cum[-1])]),
                      "n90": int(desc[np.argmax(100 * cum >= 90 * cum[-1])]), "sum_bases": int(nb.sum()), "min_bases": int(nb.min()), "max_bases": int(nb.max())}
        LC.first_diff(t.get_lengths(rs.HQ).tolist(), hq.tolist(), cap * threads, "the masked lengths")
        LC.first_diff(t.get_lengths(rs.BASES).tolist(), nb.tolist(), cap * threads, "the masked bases")
        LC.first_diff(t.get_lengths(rs.LEN_ALL).tolist(), (end - start).tolist(), cap * threads, "the lengths of every row")
        edges = np.arange(0, 100, 7)
        assert t.hist(rs.HQ, edges).tolist() == np.histogram(hq, bins=edges)[0].tolist()
    LC.timed("StsTable + lengths", t0)


@functools.lru_cache(maxsize=None)
def many_groups():
    cap, block = LC.header_define("LQ_BOX_MAX_BLOCKS"), LC.header_define("LQ_BOX_THREADS")
    n_groups = cap * block + 130
    rng = np.random.default_rng(6)
    key = rng.permutation(np.concatenate([np.arange(n_groups) * 3, rng.integers(0, n_groups, 900) * 3])).astype(np.uint32)      # (gaps; some groups of two or more)
    x = np.round(rng.normal(0.0, 2.0, key.size), 2)
    key.setflags(write=False); x.setflags(write=False)
    order = np.lexsort((x, key))
    ks, xs = key[order], x[order]
    cuts = np.flatnonzero(np.diff(ks)) + 1
    want = [dict(TB.box_of(v), group=int(v_key), n=int(v.size)) if v.size > 1 else
            dict({k: float(v[0]) for k in ("q1", "med", "q3", "whislo", "whishi", "median")}, fliers=[], group=int(v_key), n=1)
            for v_key, v in zip(ks[np.concatenate([[0], cuts])].tolist(), np.split(xs, cuts))]
    return key, x, want


def check_groups_past_cap(lib):
    cap, block = LC.header_define("LQ_BOX_MAX_BLOCKS"), LC.header_define("LQ_BOX_THREADS")
    t0 = time.time()
    key, x, want = many_groups()
    LC.assert_past_cap("k_boxd_keys / k_boxd_rekey / k_boxd_flags, elements", key.size, cap * block, block)
    LC.assert_past_cap("k_boxd_stats, groups", len(want), cap * block, block)
    LC.timed("box input (%d elements, %d groups)" % (key.size, len(want)), t0)
    t0 = time.time()
    got = rs.box_stats_f64(key, x, lib=lib)
    LC.timed("lqfig_boxstats_f64", t0)
    assert got["group"].tolist() == [b["group"] for b in want] and got["n"].tolist() == [b["n"] for b in want]
    for k in ("q1", "med", "q3", "whislo", "whishi", "median"):
        LC.first_diff(got[k].tolist(), [b[k] for b in want], cap * block, k)
    assert [sorted(f.tolist()) for f in got["fliers"]] == [sorted(b["fliers"]) for b in want]


def test_emulated_table_past_the_cap(emu_lib):
    check_table_past_cap(emu_lib)


def test_emulated_groups_past_the_cap(emu_lib):
    check_groups_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_table_past_the_cap(gpu_lib):
    check_table_past_cap(gpu_lib)


@pytest.mark.gpu
def test_gpu_groups_past_the_cap(gpu_lib):
    check_groups_past_cap(gpu_lib)

"""The walk stage of the Sequel platform QC (lqpol_add_items -> lqpol_finish -> the per-ZMW arrays: k_pol_keys, the two radix passes,
k_pol_order, k_pol_heads, k_pol_walk, k_pol_pack, k_pol_nxx of kernels_polread.hpp) against what the reference's own construct_polread,
get_N50 and get_NXX returned (tests/golden/polread.json, written by tests/golden/make_polread_golden.py) and against `model`, the same
pass restated here in plain Python.  Integers throughout: every comparison is for equality.  Under the wave emulator in its three thread
orders, and on the GPU."""
import numpy as np
import pytest

from longqc_amd import api, sequel
from tests import polread_cases
from tests import test_launch_caps as LC

GOLD = polread_cases.load()
LONG = LC.header_define("LQ_POL_LONG_ITEMS")
THREADS = LC.header_define("LQ_POL_THREADS")


def model(items):
    """(hq, tot, is_pol, ad_num) of one ZMW's items in arrival order"""
    prev_end, hs, he, hq, tot, ad, pol = 0, -1, -1, 0, 0, 0, False
    for s, e, c in sorted(items, key=lambda i: (i[0], i[1])):          # (stable: ties keep their arrival order)
        if prev_end != 0 and prev_end != s:
            gap = s - prev_end - 1
            if hs >= 0:
                hq -= gap
            tot += gap
        prev_end = e
        if c == "L":
            if hs >= 0:
                hq += he - hs
                hs = he = -1
        else:
            if hs < 0:
                hs = s
            he = e
            pol = pol or c == "S"
            ad += c == "A"
        tot += e - s
    if hs >= 0:
        hq += he - hs
    return (hq + 1 if hq > 0 else hq, tot + 1, pol, ad)


def walk(lib, groups, calls=1):
    """groups: [(zmw, items)], added ZMW after ZMW in `calls` pieces -> (PolymeraseReads after finish, {zmw: (hq, tot, is_pol, ad_num)})"""
    flat = [(z, s, e, c) for z, items in groups for s, e, c in items]
    p = sequel.PolymeraseReads(lib=lib)
    cuts = [len(flat) * k // calls for k in range(calls + 1)]
    for a, b in zip(cuts, cuts[1:]):
        if b > a:
            z, s, e, c = zip(*flat[a:b])
            p.add_items(z, s, e, "".join(c))
    sequel._finish_lenient(p)
    got = {int(z): (int(h), int(t), bool(i), int(a)) for z, h, t, i, a in zip(p.all_zmw, p.all_hq, p.all_tot, p.is_pol, p.all_ad_num)}
    assert list(p.all_zmw) == sorted(got) and len(got) == len(p.all_zmw)      # ascending, each once
    return p, got


def check_golden_units(lib):
    units = GOLD["units"]
    for u in units:                                                 # the model is the reference's function on everything recorded
        assert list(model([tuple(i) for i in u["items"]])) == u["expect"], u["name"]
    for calls in (1, 3):
        p, got = walk(lib, [(7 * k + 1, [tuple(i) for i in u["items"]]) for k, u in enumerate(units)], calls)
        for k, u in enumerate(units):
            assert list(got[7 * k + 1]) == u["expect"], (u["name"], got[7 * k + 1], u["expect"])
        assert len(got) == len(units)
        bad = sum(1 for u in units if u["expect"][2] and u["expect"][1] == 0)
        assert p.stats["n_tot_zero"] == bad and bad >= 1                # the is_pol ZMW with tot == 0 is flagged
        assert p.stats["n_out_of_range"] == sum(1 for u in units if u["expect"][2] and (u["expect"][0] < 0 or u["expect"][1] < 0)) >= 1


def check_shapes(lib, monkeypatch):
    rng = np.random.default_rng(3)

    def chain(n, start=0):
        out, pos = [], start
        for k in range(n):
            ln = int(rng.integers(0, 50))
            out.append((pos, pos + ln, "ALSSF"[int(rng.integers(0, 5))]))
            pos += ln + int(rng.integers(0, 2)) * 7
        order = rng.permutation(n)
        return [out[i] for i in order]

    # one ZMW with one item
    p, got = walk(lib, [(0, [(5, 50, "S")])])
    assert got == {0: (46, 46, True, 0)} and p.stats["n_long_zmw"] == 0
    assert (p.stats["sum_hq"], p.stats["max_hq"], p.stats["n50"], p.stats["n90"], p.stats["min_tot"], p.stats["max_tot"]) == (46, 46, 46, 46, 46, 46)
    # nothing at all
    p, got = walk(lib, [])
    assert got == {} and p.n_pol == 0
    # the long-ZMW path: LONG items stay in the first launch, LONG + 1 go to the second; short ZMWs around them
    for n_long_items, want in ((LONG, 0), (LONG + 1, 1), (3 * LONG + 5, 1)):
        groups = [(3, chain(4)), (900000000, chain(n_long_items)), (900000001, chain(2)), (1, chain(1))]
        p, got = walk(lib, groups, calls=2)
        assert got == {z: model(items) for z, items in groups}
        assert p.stats["n_long_zmw"] == want
    # ZMW counts around one block, and past a launch cap of two blocks: cap + 1 groups
    monkeypatch.setenv("LQPOL_TEST_MAX_BLOCKS", "2")
    for n in (THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1):
        groups = [(int(z), chain(1 + k % 3)) for k, z in enumerate(rng.choice(10 ** 9, n, replace=False))]
        p, got = walk(lib, groups)
        assert got == {z: model(items) for z, items in groups}, n
    monkeypatch.delenv("LQPOL_TEST_MAX_BLOCKS")
    # a ZMW split across three calls, its items interleaved with another's in arrival order
    a, b = chain(30), chain(31)
    flat = [(11, *a[k // 2]) if k % 2 == 0 else (12, *b[k // 2]) for k in range(60)] + [(12, *b[30])]
    p = sequel.PolymeraseReads(lib=lib)
    for part in (flat[:20], flat[20:41], flat[41:]):
        z, s, e, c = zip(*part)
        p.add_items(z, s, e, "".join(c))
    sequel._finish_lenient(p)
    assert (int(p.all_hq[0]), int(p.all_tot[0]), bool(p.is_pol[0]), int(p.all_ad_num[0])) == model(a)
    assert (int(p.all_hq[1]), int(p.all_tot[1]), bool(p.is_pol[1]), int(p.all_ad_num[1])) == model(b)
    # ZMWs that differ only above bit 24, start and end at the top of the domain
    base = 0x3f0041
    groups = [(base + (k << 24), [(999999990 - k, 999999999, "S"), (0, 999999999, "A"), (999999999, 999999999, "L")]) for k in (3, 0, 2, 1)]
    p, got = walk(lib, groups)
    assert got == {z: model(items) for z, items in groups} and len(got) == 4
    # ties between an L and another class at equal (start, end): the arrival order decides
    first = [(0, 40, "S"), (40, 90, "L"), (40, 90, "A"), (90, 200, "S")]
    last = [(0, 40, "S"), (40, 90, "A"), (40, 90, "L"), (90, 200, "S")]
    p, got = walk(lib, [(1, first), (2, last)])
    assert got[1] == model(first) and got[2] == model(last) and got[1] != got[2]
    # outside the domain
    p = sequel.PolymeraseReads(lib=lib)
    with pytest.raises(api.LqcovError) as e:
        p.add_items([1], [0], [10 ** 9], "S")
    assert e.value.code == -5


def check_nxx(lib):
    for case in GOLD["nxx"]:
        vals = case["vals"]
        assert all(v == 0 or v >= 2 for v in vals)
        groups = [(1000 - k, [(0, v - 1, "S")] if v else [(0, 0, "S")]) for k, v in enumerate(vals)]
        p, got = walk(lib, groups)
        assert sorted(g[0] for g in got.values()) == sorted(vals)
        assert (float(p.stats["n50"]), float(p.stats["n90"])) == (case["n50"], case["n90"]), vals
        assert p.stats["sum_hq"] == sum(vals) and p.stats["max_hq"] == max(vals)
        assert sorted(p.hr_lengths.tolist()) == sorted(vals)


CHECKS = [check_golden_units, check_nxx]


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_walk_equals_the_reference(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_golden_units(emu_lib)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_walk_shapes(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_shapes(emu_lib, monkeypatch)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_nxx_equals_get_nxx(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_nxx(emu_lib)


def test_polymerase_reads_takes_the_issue_table(emu_lib):
    items = {k + 1: [tuple(i) for i in u["items"]] for k, u in enumerate(GOLD["units"][:6])}
    got = sequel.polymerase_reads(items, lib=emu_lib)
    assert [list(got[k + 1]) for k in range(6)] == [[1901, 2501, True, 2], [182, 90, True, 1], [31, 90, False, 0], [57, 119, True, 0], [46, 46, True, 0], [0, 1, True, 0]]


@pytest.mark.gpu
def test_gpu_walk_equals_the_reference(gpu_lib, monkeypatch):
    check_golden_units(gpu_lib)
    check_nxx(gpu_lib)
    check_shapes(gpu_lib, monkeypatch)

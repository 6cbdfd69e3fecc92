"""The k_pol_* kernels past their launch caps (kernels_polread.hpp), after the scheme of tests/test_launch_caps.py: the smallest inputs
that make every one of them run its grid-stride loop a second time -- more record tiles than k_pol_fields and k_pol_compact have blocks
(one scan of one range of bytes), more items than one round of k_pol_keys, k_pol_rekey, k_pol_order and k_pol_heads takes, more ZMWs than
one round of k_pol_walk, k_pol_ispol and k_pol_pack, more polymerase reads than one round of k_pol_unkey and k_pol_nxx -- with partial last
units.  Caps and tiles are read from the header; the expected values come from `model` (tests/test_polread_walk.py) and from numpy."""
import time

import numpy as np
import pytest

from longqc_amd import sequel
from tests import bam_writer as BW
from tests import test_launch_caps as LC
from tests.test_polread_fields import HDR, ITEM, fields
from tests.test_polread_walk import model


def tiny_records(n, rng):
    """n scraps records of l_seq 0 with sz N and a class: -> (the bytes, zmw, start, end, class arrays)"""
    zmw, start = rng.integers(0, n // 3 + 1, n), rng.integers(0, 2000, n)
    end, cls = start + rng.integers(0, 50, n), np.frombuffer(b"ALFB", np.uint8)[rng.integers(0, 4, n)]
    parts = [HDR]
    for z, s, e, c in zip(zmw.tolist(), start.tolist(), end.tolist(), cls.tolist()):
        parts.append(BW.record(b"m/%d/%d_%d" % (z, s, e), b"", None, tags=b"szANscA" + bytes([c])))
    return b"".join(parts), zmw, start, end, cls


def check_fields_past_cap(lib):
    cap, ltile = LC.header_define("LQ_POL_MAX_BLOCKS"), LC.header_define("LQ_FXSCAN_LINE_TILE")
    t0 = time.time()
    n = (cap + 101) * ltile + 17
    data, zmw, start, end, cls = tiny_records(n, np.random.default_rng(4))
    LC.assert_past_cap("k_pol_fields / k_pol_compact, record tiles", (n + ltile - 1) // ltile, cap)
    assert n % ltile != 0
    LC.timed("fields input (%d records, %d bytes)" % (n, len(data)), t0)
    t0 = time.time()
    flags, slots, control, resume = fields(lib, 0, data)
    LC.timed("lqpol_fields", t0)
    assert resume == len(data) and control == 0
    assert np.array_equal(np.array(flags, np.uint32), np.full(n, ITEM, np.uint32))
    assert np.array_equal(np.array(slots, np.int64), np.stack([zmw, start, end, cls], axis=1))


def check_walk_past_cap(lib):
    cap, threads = LC.header_define("LQ_POL_MAX_BLOCKS"), LC.header_define("LQ_POL_THREADS")
    rng = np.random.default_rng(6)
    t0 = time.time()
    n_zmw = cap * threads + 60 * threads + 11                          # every twentieth ZMW without a subread: still more than cap * threads with one
    zmws = rng.choice(10 ** 9, n_zmw, replace=False)
    items = []
    for k, z in enumerate(zmws.tolist()):
        s = k % 7
        items.append((z, s, s + 2 + k % 90, "S" if k % 20 else "A"))
        if k % 2:
            items.append((z, s + 2 + k % 90, s + 100, "ALF"[k % 3]))
    order = rng.permutation(len(items))
    items = [items[i] for i in order.tolist()]
    per_zmw = {}
    for z, s, e, c in items:
        per_zmw.setdefault(z, []).append((s, e, c))
    n_pol = sum(1 for l in per_zmw.values() if any(c == "S" for _, _, c in l))
    LC.assert_past_cap("k_pol_keys / k_pol_rekey / k_pol_order / k_pol_heads, items", len(items), cap * threads, threads)
    LC.assert_past_cap("k_pol_walk / k_pol_ispol / k_pol_pack, ZMWs", n_zmw, cap * threads, threads)
    LC.assert_past_cap("k_pol_unkey / k_pol_nxx, polymerase reads", n_pol, cap * threads, threads)
    LC.timed("walk input (%d items, %d ZMWs)" % (len(items), n_zmw), t0)
    t0 = time.time()
    p = sequel.PolymeraseReads(lib=lib)
    z, s, e, c = zip(*items)
    p.add_items(z, s, e, "".join(c))
    p.finish()
    LC.timed("lqpol_add_items + lqpol_finish", t0)
    want = sorted((z,) + model(l) for z, l in per_zmw.items())
    got = list(zip(p.all_zmw.tolist(), p.all_hq.tolist(), p.all_tot.tolist(), p.is_pol.tolist(), p.all_ad_num.tolist()))
    LC.first_diff(got, want, cap * threads, "the per-ZMW results")
    hq = np.array(sorted((w[1] for w in want if w[3]), reverse=True), np.int64)
    cum = np.cumsum(hq)
    assert p.n_pol == n_pol == hq.size and p.stats["sum_hq"] == int(cum[-1]) and p.stats["max_hq"] == int(hq[0])
    assert p.stats["n50"] == int(hq[np.argmax(2 * cum >= cum[-1])]) and p.stats["n90"] == int(hq[np.argmax(100 * cum >= 90 * cum[-1])])
    assert p.ad_num_stat == {int(a): int(n) for a, n in zip(*np.unique([w[4] for w in want if w[3]], return_counts=True))}


def test_emulated_fields_past_the_cap(emu_lib):
    check_fields_past_cap(emu_lib)


def test_emulated_walk_past_the_cap(emu_lib):
    check_walk_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_fields_past_the_cap(gpu_lib):
    check_fields_past_cap(gpu_lib)


@pytest.mark.gpu
def test_gpu_walk_past_the_cap(gpu_lib):
    check_walk_past_cap(gpu_lib)

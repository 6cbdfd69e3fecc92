"""The table's kernels past their launch cap (kernels_dust_table.hpp), after the scheme of tests/test_fastq_out_caps.py: the smallest seeded
set of rows that exceeds block cap x threads of k_sdust_rows and k_sdust_text by at least 100 rows, so that lanes run their loop a second
time -- the loop increment, the partial last block, the sums a lane carries from its first row to its second, the atomics of the lists.
With window = 1 every row with qualities is on the unvouched list, whose length then exceeds k_sdust_patch's launch in the same way.  The
cap and the thread count are read from the header.  The rows go through lqsdust_format, so nothing is scanned; the second round mixes
empty names, 40-byte names and "-nan" rows; the reference is sdust._rows."""
import time

import numpy as np
import pytest

from longqc_amd import sdust
from tests import test_launch_caps as LC
from tests import test_sdust_table as ST


def caps_rows(seed):
    threads, cap = LC.header_define("LQ_DTAB_THREADS"), LC.header_define("LQ_DTAB_MAX_BLOCKS")
    per_round = threads * cap
    n = per_round + 157                                             # (the last block of the second round is partial)
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 30000, n).astype(np.uint32)
    masked = (lens * rng.random(n)).astype(np.uint32)
    qv = (lens * rng.random(n)).astype(np.uint32)
    psum = lens * 10.0 ** (-rng.random(n) * 4)
    has_q = np.ones(n, np.uint8)
    names = ["r%d" % i for i in range(n)]
    second = np.arange(per_round, n)
    for i in second[::5].tolist():
        names[i] = ""
    for i in second[1::5].tolist():
        names[i] = "".join(chr(x) for x in rng.integers(48, 123, 40))
    nan_rows = second[2::7]                                         # no bases: "-nan" in both columns
    lens[nan_rows] = masked[nan_rows] = qv[nan_rows] = 0
    has_q[second[3::7]] = 0                                         # no qualities: "-nan" in the meanQ column
    lens[second[4::11]], masked[second[4::11]] = 20000, 9000        # and reads on the second exclusion list
    return names, masked, lens, psum, has_q, qv, per_round


def check_table_past_cap(lib):
    t0 = time.time()
    names, masked, lens, psum, has_q, qv, per_round = caps_rows(seed=303)
    n = len(names)
    LC.assert_past_cap("k_sdust_rows / k_sdust_text, rows", n, per_round, LC.header_define("LQ_DTAB_THREADS"))
    assert n - per_round < 200                                      # (the smallest such input)
    with_q = int(((has_q != 0) & (lens > 0)).sum())
    LC.assert_past_cap("k_sdust_patch, unvouched rows at window 1", with_q, per_round, LC.header_define("LQ_DTAB_THREADS"))
    second = slice(per_round, n)
    assert sum(x == "" for x in names[second]) >= 20 and sum(len(x) == 40 for x in names[second]) >= 20
    assert int((lens[second] == 0).sum()) >= 10 and int(((has_q[second] == 0) & (lens[second] > 0)).sum()) >= 10
    want = ST.want_text(names, masked, lens, psum, has_q, qv)
    LC.timed("rows input and _rows (%d rows, %d bytes)" % (n, len(want)), t0)
    for window, unv in ((0.0, None), (1.0, with_q)):
        t0 = time.time()
        got, st = sdust.format_rows(names, masked, lens, psum, has_q, qv, window=window, lib=lib)
        LC.timed("lqsdust_format, window %g" % window, t0)
        ST.assert_same_text(got, want)
        assert st["rows"] == n and st["bytes"] == len(want) and st["masked"] == int(masked.sum(dtype=np.uint64)) and st["q7"] == int(qv.sum(dtype=np.uint64))
        assert st["unvouched"] == unv if unv is not None else st["unvouched"] <= n // 100
        assert st["excluded_first"] == 0 and st["excluded"] == len(sdust.exclusion_lists(masked, lens)[1]) >= 10


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_table_past_the_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_table_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_table_past_the_cap(gpu_lib):
    check_table_past_cap(gpu_lib)

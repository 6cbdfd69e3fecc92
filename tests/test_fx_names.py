"""k_fx_names (kernels_fxscan.hpp) through chunkpass.gather_names against Python slicing of the rows chunkpass.scan_records gives: the
blob is every name followed by one NUL, the offsets are the prefix sums of name length + 1, first_bad is the first row whose name
holds a byte of 0x80 or more."""
import random

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_launch_caps as LC

THREADS = LC.header_define("LQ_FXSCAN_THREADS")
MAX_BLOCKS = LC.header_define("LQ_FXSCAN_MAX_BLOCKS")


def check_names(lib, data, rows, want_n=None):
    rows = np.asarray(rows, np.uint32).reshape(-1, 4)
    n = rows.shape[0]
    if want_n is not None:
        assert n == want_n, (n, want_n)
    names = [data[int(a):int(a) + int(l)] for a, l in rows[:, :2].tolist()]
    blob, off, first_bad = chunkpass.gather_names(data, rows, lib=lib)
    assert blob == b"".join(x + b"\0" for x in names)
    assert off.tolist() == np.concatenate(([0], np.cumsum([len(x) + 1 for x in names]))).astype(np.uint64).tolist()
    assert first_bad == next((i for i, x in enumerate(names) if any(c >= 0x80 for c in x)), n)
    return names


def fastq(names, rng, eol=b"\n"):
    out = bytearray()
    for nm in names:
        l = rng.randrange(1, 40)
        out += b"@" + nm + eol + bytes(rng.choices(b"ACGT", k=l)) + eol + b"+" + eol + b"I" * l + eol
    return bytes(out)


def check_scanned(lib):
    rng = random.Random(3)
    # empty names, names with comments behind them, one record
    for hdrs, want in (([b"r1", b"", b"r3 comment here", b"r4\tc", b"", b"x" * 300 + b" y"], [b"r1", b"", b"r3", b"r4", b"", b"x" * 300]),
                       ([b"only"], [b"only"]), ([b""], [b""])):
        data = fastq(hdrs, rng)
        rows = chunkpass.scan_records(data, lib=lib)[0]
        assert check_names(lib, data, rows, len(hdrs)) == want
    # CRLF headers: the '\r' ends the name
    data = fastq([b"a1", b"b2 c", b""], rng, eol=b"\r\n")
    rows = chunkpass.scan_records(data, lib=lib)[0]
    assert check_names(lib, data, rows, 3) == [b"a1", b"b2", b""]
    # more rows than one block has lanes
    hdrs = [b"read/%d/%s" % (i, b"z" * (i % 7)) for i in range(THREADS * 2 + 37)]
    data = fastq(hdrs, rng)
    rows = chunkpass.scan_records(data, lib=lib)[0]
    assert check_names(lib, data, rows, len(hdrs)) == hdrs
    # a parser that stands behind a header character
    rows = chunkpass.scan_records(data, 1, ord("@"), lib=lib)[0]
    assert check_names(lib, data, rows, len(hdrs)) == hdrs
    assert chunkpass.gather_names(b"", np.zeros((0, 4), np.uint32), lib=lib) == (b"", [0], 0)


def check_first_bad(lib):
    rng = random.Random(5)
    hdrs = [b"n%d" % i for i in range(THREADS + 9)]
    for bad in ([0], [len(hdrs) - 1], [], [260, 17, 200]):
        h = list(hdrs)
        for i in bad:
            h[i] = b"n\x80%d" % i if i % 2 else b"\xffn%d" % i
        data = fastq(h, rng)
        rows = chunkpass.scan_records(data, lib=lib)[0]
        assert check_names(lib, data, rows, len(h)) == h
        assert chunkpass.gather_names(data, rows, lib=lib)[2] == (min(bad) if bad else len(h))


def check_names_past_cap(lib):
    """more tiles of rows than a launch has workgroups, at the smallest shape: the rows point into a few bytes over and over"""
    n = MAX_BLOCKS * THREADS + 107 * THREADS + 11
    LC.assert_past_cap("k_fx_names, rows", n, MAX_BLOCKS * THREADS, THREADS)
    data = b"@ab\n@\n@cdefg h\n@\x80\n"
    pick = np.array([[1, 2, 0, 0], [5, 0, 0, 0], [7, 5, 0, 0]], np.uint32)
    rows = pick[np.arange(n) % 3]
    rows[-5] = [16, 1, 0, 0]                                        # the byte of 0x80, in the second round
    names = [data[int(a):int(a) + int(l)] + b"\0" for a, l in pick[:, :2].tolist()]
    blob, off, first_bad = chunkpass.gather_names(data, rows, lib=lib)
    lens = rows[:, 1].astype(np.uint64) + 1
    assert (off == np.concatenate(([0], np.cumsum(lens)))).all()
    want = np.frombuffer(b"".join(names) * (n // 3 + 1), np.uint8)[:int(off[n - 5])]
    got = np.frombuffer(blob, np.uint8)
    assert (got[:want.shape[0]] == want).all()
    assert blob[int(off[n - 5]):] == b"\x80\0" + b"".join(names[(n - 4 + k) % 3] for k in range(4))
    assert first_bad == n - 5


def test_emulated_names_of_scanned_rows(emu_lib):
    check_scanned(emu_lib)


def test_emulated_names_first_bad(emu_lib):
    check_first_bad(emu_lib)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_names_past_the_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_names_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_names_of_scanned_rows(gpu_lib):
    check_scanned(gpu_lib)


@pytest.mark.gpu
def test_gpu_names_first_bad(gpu_lib):
    check_first_bad(gpu_lib)


@pytest.mark.gpu
def test_gpu_names_past_the_cap(gpu_lib):
    check_names_past_cap(gpu_lib)

"""k_gz_find, k_gz_inflate_spec and k_gz_resolve past their launch cap (kernels_gzip.hpp), after tests/test_inflate_caps.py: more
non-empty spans in one launch than the launch has workgroups, at the smallest shape -- spans of 1024 compressed bytes of a memLevel-3
stream of reads with random qualities, which has a dynamic block about every 700 bytes, so that nearly every span is found, decoded and accepted and the first
workgroups run their loop a second time: the loop increment, the ring and the tables of LDS used again, the report of the second
round.  One launch must have accepted more spans than the cap; the bytes are zlib's."""
import random
import zlib

import pytest

from longqc_amd import chunkpass
from tests import test_launch_caps as LC


def check_gzip_past_cap(lib):
    cap = LC.header_define("LQ_GZ_MAX_BLOCKS")
    rng = random.Random(43)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(rng.choices(b"ACGT", k=300)), bytes(rng.choices(b"#$%&'()*+,-./0123456789:;", k=300))) for i in range(1900))
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 3)
    comp = c.compress(text) + c.flush()
    n_spans = len(comp) // 1024
    LC.assert_past_cap("k_gz_*, spans", n_spans, cap)
    got, st = chunkpass.inflate_gzip(comp, 1024, lib=lib, out_cap=4 * len(text))      # (room for the whole file: one window)
    print(len(text), len(comp), st)
    assert got == text
    # more accepted spans than every launch's first round takes together: one launch at least went into its second round
    assert st["spans_accepted"] >= st["launches"] * cap + 100 and st["bytes_zlib"] == 0, st


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_gzip_past_the_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_gzip_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_gzip_past_the_cap(gpu_lib):
    check_gzip_past_cap(gpu_lib)

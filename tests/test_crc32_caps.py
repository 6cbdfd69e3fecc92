"""k_crc32_ranges past its launch cap (kernels_crc32.hpp), after tests/test_inflate_caps.py: more ranges than one launch has
workgroups, at the smallest shape -- LQ_CRC_MAX_BLOCKS + 107 ranges of 37 bytes (the last one of 11), back to back, so that the first
workgroups run their loop a second time with the tables of LDS they made once; every range of the second round is compared with
zlib.crc32."""
import random
import zlib

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_launch_caps as LC


def check_crc32_past_cap(lib):
    cap = LC.header_define("LQ_CRC_MAX_BLOCKS")
    n = cap + 107
    LC.assert_past_cap("k_crc32_ranges, ranges", n, cap)
    rng = random.Random(43)
    length = [37] * (n - 1) + [11]                                  # the last one is partial
    off = np.concatenate(([3], 3 + np.cumsum(length[:-1]))).tolist()
    data = rng.randbytes(off[-1] + length[-1] + 5)
    assert len({x % 16 for x in off[cap:]}) == 16
    got = chunkpass.crc32_ranges(data, off, length, lib=lib)
    bad = [i for i in range(n) if int(got[i]) != zlib.crc32(data[off[i]:off[i] + length[i]])]
    assert not bad, "ranges differ: %s (the second round begins at %d)" % (bad[:10], cap)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_crc32_past_the_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_crc32_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_crc32_past_the_cap(gpu_lib):
    check_crc32_past_cap(gpu_lib)

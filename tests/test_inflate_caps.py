"""k_bgzf_inflate past its launch cap (kernels_inflate.hpp), after tests/test_bamchunks_caps.py: more members than one launch has
workgroups, at the smallest shape -- LQ_INFLATE_MAX_BLOCKS + 107 members of 37 payload bytes (the last one of 11) at mixed levels and
strategies, so that the first workgroups run their loop a second time: the loop increment, the history and the tables of LDS used
again, the status of the second round.  Every member a workgroup takes in its second round is compared with the bytes compressed."""
import random
import zlib

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_launch_caps as LC


def check_inflate_past_cap(lib):
    cap = LC.header_define("LQ_INFLATE_MAX_BLOCKS")
    n = cap + 107
    LC.assert_past_cap("k_bgzf_inflate, members", n, cap)
    rng = random.Random(41)
    pay = [bytes(rng.choices(b"ACGT", k=37)) if i % 3 else rng.randbytes(37) if i % 2 else b"AC" * 18 + b"A" for i in range(n)]
    pay[-1] = pay[-1][:11]                                          # the last one is partial
    comp, in_off, in_len, out_off, o = bytearray(), [], [], [], 0
    for i, p in enumerate(pay):
        c = zlib.compressobj((0, 1, 6, 9)[i % 4], zlib.DEFLATED, -15, 9, (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY)[i // 4 % 3])
        d = c.compress(p) + c.flush()
        in_off.append(len(comp)); in_len.append(len(d)); out_off.append(o)
        comp += d
        o += len(p)                                                 # back to back, as the members of a file land in the piece
    got, status = chunkpass.inflate_blocks(bytes(comp), in_off, in_len, out_off, [len(p) for p in pay], out=np.full(o + 16, 0xEE, np.uint8), lib=lib)
    assert (status == 0).all(), np.flatnonzero(status)[:10]
    assert len({x % 16 for x in out_off[cap:]}) == 16
    bad = [i for i in range(n) if got[out_off[i]:out_off[i] + len(pay[i])].tobytes() != pay[i]]
    assert not bad, "members differ: %s (the second round begins at %d)" % (bad[:10], cap)
    assert (got[o:] == 0xEE).all()


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_inflate_past_the_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_inflate_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_inflate_past_the_cap(gpu_lib):
    check_inflate_past_cap(gpu_lib)

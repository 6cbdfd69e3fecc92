"""k_bam_gather past its launch cap (kernels_bam.hpp), after tests/test_filechunks_caps.py: the smallest seeded BAM whose bases fill
more tiles of destination bytes than one launch has blocks, so that every block runs its loop a second time -- the loop increment,
the partial last tile, the per-tile segment table of the second round, both nibble parities there.  The cap and the tile are read
from the header.  The reference is the decode restated in numpy on the inflated bytes: base i of the flat buffer is the high (even
i - dst[s]) or the low nibble of byte src[s] + (i - dst[s]) // 2 of the read s that holds it, looked up in "=ACMGRSVTWYHKDBN"."""
import struct
import time

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import bam_writer as BW
from tests import test_launch_caps as LC

TABLE = np.frombuffer(BW.CODES, dtype=np.uint8)


def caps_input(seed):
    """-> (inflated bytes, lens, segs: (src, dst, len) of every read's packed sequence): reads of 2000..9000 bases, runs of 0..100-base
    reads between them, two empty reads at the end; names and tag blobs of varying length put the sequences at every residue"""
    tile, cap = LC.header_define("LQ_GATHER_TILE"), LC.header_define("LQ_GATHER_MAX_BLOCKS")
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < (cap + 101) * tile:
        lens += [int(rng.integers(2000, 9001))] + [int(x) for x in rng.integers(0, 101, int(rng.integers(0, 8)))]
    lens = np.array(lens + [51, 0, 0], dtype=np.int64)
    if lens.sum() % tile == 0:
        lens[-3] += 2
    n = lens.shape[0]
    nibbles = rng.integers(0, 16, int(lens.sum())).astype(np.uint8)
    parts, segs, at, d = [BW.header()], [], len(BW.header()), 0
    for r, l in enumerate(lens.tolist()):
        nb = nibbles[d:d + l]
        if l & 1:
            nb = np.append(nb, np.uint8(0))
        packed = (nb[0::2] << 4 | nb[1::2]).astype(np.uint8).tobytes()
        name = b"r%d" % r + b"/" * (r % 5) + b"\0"
        tags = b"\xfe" * int(rng.integers(0, 12))
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 0, 4680, 0, 4, l, -1, -1, 0) + name + packed + b"\xff" * l + tags
        segs.append((at + 4 + 32 + len(name), d, l))
        parts.append(struct.pack("<i", len(body)) + body)
        at += 4 + len(body); d += l
    return b"".join(parts), lens, np.array(segs, dtype=np.int64), TABLE[nibbles]


def numpy_decode(data, segs, total):
    src, dst, ln = segs[:, 0], segs[:, 1], segs[:, 2]
    assert (dst[1:] == dst[:-1] + ln[:-1]).all() and dst[0] == 0 and dst[-1] + ln[-1] == total      # no gaps
    s = np.repeat(np.arange(segs.shape[0]), ln)
    k = np.arange(total) - dst[s]
    byte = data[src[s] + k // 2]
    return TABLE[np.where(k % 2 == 0, byte >> 4, byte & 15)]


def check_bam_gather_past_cap(lib, tmp_path):
    tile, cap = LC.header_define("LQ_GATHER_TILE"), LC.header_define("LQ_GATHER_MAX_BLOCKS")
    t0 = time.time()
    stream, lens, segs, letters = caps_input(seed=211)
    data = np.frombuffer(stream, dtype=np.uint8)
    total, n = int(lens.sum()), lens.shape[0]
    n_tiles = (total + tile - 1) // tile
    LC.assert_past_cap("k_bam_gather, tiles", n_tiles, cap)
    assert total % tile != 0                                        # the last tile is partial
    assert n_tiles - cap < 110                                      # (the smallest such input)
    long_reads = lens[lens >= 2000]
    assert (long_reads % 2 == 0).any() and (long_reads % 2 == 1).any()
    # the second round: whole reads that start there at both parities of the destination (so lanes start inside reads at odd and at
    # even bases), every residue of the source and of the destination
    hdr = len(BW.header())
    second = segs[(segs[:, 1] >= cap * tile) & (segs[:, 2] > 0)]
    assert (second[:, 2] >= 2000).sum() >= 3 and (second[:, 2] <= 100).sum() >= 100
    word = np.arange(cap * tile, total, 16)                         # the first base of every lane of the second round
    s = np.searchsorted(segs[:, 1], word, side="right") - 1
    assert set(((word - segs[s, 1]) % 2).tolist()) == {0, 1}        # both start parities
    assert set((second[:, 0] % 16).tolist()) == set(range(16)) == set(((second[:, 0] - hdr) % 16).tolist())
    assert set((second[:, 1] % 16).tolist()) == set(range(16))
    assert (lens[-2:] == 0).all() and (lens == 0).sum() > 10
    want = numpy_decode(data, segs, total)
    assert (want == letters).all() and set(want.tolist()) == set(BW.CODES)
    path = str(tmp_path / "caps.bam")
    with open(path, "wb") as f:
        f.write(BW.bgzf(stream, 65280, 1))
    LC.timed("BAM input (%d reads, %d bases, %d inflated bytes, %d tiles)" % (n, total, len(stream), n_tiles), t0)
    t0 = time.time()
    L = chunkpass._lib(lib)
    got = []
    for ch, n_seqs, n_bases in chunkpass.FileChunks(path, chunk_size=1 << 40, lib=lib):
        assert (ch.n, n_seqs, n_bases) == (n, n, total) and (ch.lens == lens).all() and ch.names[-1] == "r%d%s" % (n - 1, "/" * ((n - 1) % 5))
        g_seq, g_qual = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        assert L.lqchunk_get_reads(ch.h, 0, None, g_seq.ctypes.data, g_qual.ctypes.data) == 0
        got.append((g_seq, g_qual))
    LC.timed("FileChunks + lqchunk_get_reads", t0)
    assert len(got) == 1
    for g, w, what in ((got[0][0], want, "sequences"), (got[0][1], np.full(total, 33, np.uint8), "qualities")):
        bad = np.flatnonzero(g != w)
        assert bad.shape[0] == 0, "%s: %d bytes differ, first at %s relative to the second round's first byte (%d): %s != %s" % (
            what, bad.shape[0], bad[:5] - cap * tile, cap * tile, g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_bam_gather_past_the_cap(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_bam_gather_past_cap(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_bam_gather_past_the_cap(gpu_lib, tmp_path):
    check_bam_gather_past_cap(gpu_lib, tmp_path)

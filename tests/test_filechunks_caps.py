"""k_chunk_gather past its launch cap (kernels_gather.hpp), after the scheme of tests/test_launch_caps.py: the smallest seeded FASTQ
whose sequences fill more tiles of destination bytes than one launch has blocks, so that every block runs its loop a second time --
the loop increment, the partial last tile, the per-tile segment table of the second round.  The cap and the tile are read from the
header; the check asserts that the shape exceeds the cap, that at least 100 tiles fall into the second round and that the last tile is
partial.  The reference is the gather restated in numpy on the file's bytes: destination byte i of a buffer is source byte
src[s] + i - dst[s] of the segment s that holds it."""
import ctypes as C
import time

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_launch_caps as LC

ALPHABET = np.frombuffer(b"ACGTacgtNnUu", dtype=np.uint8)


def caps_input(seed):
    """-> (file bytes, lens, sseg, qseg): reads of 2000..9000 bases wrapped at 60, at 61 and on one line, runs of short reads (0..100
    bases, one line) between them; sseg / qseg: (src, dst, len) of every line of the sequences / of the quality strings"""
    tile, cap = LC.header_define("LQ_GATHER_TILE"), LC.header_define("LQ_GATHER_MAX_BLOCKS")
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < (cap + 101) * tile:
        lens += [int(rng.integers(2000, 9001))] + [int(x) for x in rng.integers(0, 101, int(rng.integers(0, 8)))]
    lens = np.array(lens + [50, 0, 0], dtype=np.int64)
    if lens.sum() % tile == 0:
        lens[-3] += 1
    total = int(lens.sum())
    seq = ALPHABET[rng.integers(0, ALPHABET.shape[0], total)]
    qual = rng.integers(33, 127, total).astype(np.uint8)
    parts, sseg, qseg, at, d = [], [], [], 0, 0

    def lines(buf, a, n, width, segs):
        nonlocal at
        if n == 0:
            parts.append(b"\n"); at += 1
        for i in range(0, n, width):
            m = min(width, n - i)
            segs.append((at, a + i, m))
            parts.append(buf[a + i:a + i + m].tobytes()); parts.append(b"\n")
            at += m + 1

    for r, l in enumerate(lens.tolist()):
        head = b"@r%d c\n" % r
        parts.append(head); at += len(head)
        width = (60, 61, 1 << 30)[r % 3] if l >= 2000 else 1 << 30
        lines(seq, d, l, width, sseg)
        parts.append(b"+\n"); at += 2
        lines(qual, d, l, width, qseg)
        d += l
    return b"".join(parts), lens, np.array(sseg, dtype=np.int64), np.array(qseg, dtype=np.int64), seq, qual


def numpy_gather(data, segs, total, upper):
    src, dst, ln = segs[:, 0], segs[:, 1], segs[:, 2]
    assert (dst[1:] == dst[:-1] + ln[:-1]).all() and dst[0] == 0 and dst[-1] + ln[-1] == total      # no gaps
    s = np.repeat(np.arange(segs.shape[0]), ln)
    out = data[src[s] + np.arange(total) - dst[s]]
    if upper:
        out = np.where((out >= ord("a")) & (out <= ord("z")), out - 32, out).astype(np.uint8)
    return out


def check_gather_past_cap(lib, tmp_path):
    tile, cap = LC.header_define("LQ_GATHER_TILE"), LC.header_define("LQ_GATHER_MAX_BLOCKS")
    t0 = time.time()
    raw, lens, sseg, qseg, seq, qual = caps_input(seed=101)
    data = np.frombuffer(raw, dtype=np.uint8)
    total, n = int(lens.sum()), lens.shape[0]
    n_tiles = (total + tile - 1) // tile
    LC.assert_past_cap("k_chunk_gather, tiles", n_tiles, cap)
    assert total % tile != 0                                        # the last tile is partial
    assert n_tiles - cap < 110 and len(raw) % 16384 != 0            # (the smallest such input)
    for segs in (sseg, qseg):
        second = segs[segs[:, 1] >= cap * tile]                     # lines of the second round: wrapped and whole reads, every residue
        assert (second[:, 2] == 60).sum() >= 100 and (second[:, 2] == 61).sum() >= 100 and (second[:, 2] > 1000).sum() >= 3
        assert (second[:, 2] <= 100).sum() >= 100
        assert set((second[:, 0] % 16).tolist()) == set(range(16)) and set((second[:, 1] % 16).tolist()) == set(range(16))
    assert (lens[-2:] == 0).all() and (lens == 0).sum() > 10
    w_seq, w_qual = numpy_gather(data, sseg, total, True), numpy_gather(data, qseg, total, False)
    assert (w_qual == qual).all() and (w_seq != seq).any() and seq.tobytes().upper() == w_seq.tobytes()
    path = str(tmp_path / "caps.fq")
    open(path, "wb").write(raw)
    LC.timed("gather input (%d reads, %d bases, %d file bytes, %d tiles)" % (n, total, len(raw), n_tiles), t0)
    t0 = time.time()
    L = chunkpass._lib(lib)
    got = []
    for ch, n_seqs, n_bases in chunkpass.FileChunks(path, chunk_size=1 << 40, lib=lib):
        assert (ch.n, n_seqs, n_bases) == (n, n, total) and (ch.lens == lens).all() and ch.names[-1] == "r%d" % (n - 1)
        g_seq, g_qual = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        assert L.lqchunk_get_reads(ch.h, 0, None, g_seq.ctypes.data, g_qual.ctypes.data) == 0
        got.append((g_seq, g_qual))
    LC.timed("FileChunks + lqchunk_get_reads", t0)
    assert len(got) == 1
    for g, w, what in ((got[0][0], w_seq, "sequences"), (got[0][1], w_qual, "qualities")):
        bad = np.flatnonzero(g != w)
        assert bad.shape[0] == 0, "%s: %d bytes differ, first at %s (the second round starts at byte %d): %s != %s" % (
            what, bad.shape[0], bad[:5], cap * tile, g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_gather_past_the_cap(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_gather_past_cap(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_gather_past_the_cap(gpu_lib, tmp_path):
    check_gather_past_cap(gpu_lib, tmp_path)

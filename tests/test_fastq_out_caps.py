"""k_fastq_format past its launch cap (kernels_fastq.hpp), after the scheme of tests/test_filechunks_caps.py: the smallest seeded chunk
whose text, made as one piece (lqchunk_fastq), fills more tiles than one launch has blocks, so that every block runs its loop a second
time -- the loop increment, the partial last tile, the per-tile record table of the second round.  The cap and the tile are read from
the header; the check asserts that the shape exceeds the cap, that at least 100 tiles fall into the second round, that the last tile
is partial and that the second round holds records whose start and whose fields begin at every residue mod 16.  The reference is the
text restated in bytes from the host copies of the names, bases, qualities and bounds."""
import time

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_launch_caps as LC


def caps_input(seed):
    """-> (records [name, seq, qual] of bytes, begin, end): reads of 2000..9000 bases, runs of short reads (0..100 bases) and runs of
    empty reads without a name between them (three records in one 16-byte word); every third read is cut at both ends"""
    tile, cap = LC.header_define("LQ_FASTQ_TILE"), LC.header_define("LQ_FASTQ_MAX_BLOCKS")
    rng = np.random.default_rng(seed)
    recs, begin, end, size = [], [], [], 0

    def add(l, name):
        nonlocal size
        i = len(recs)
        b, e = 0, l
        if i % 3 == 0 and l:
            b = int(rng.integers(0, min(l, 200) + 1))
            e = int(rng.integers(max(b, l - 200), l + 1))
        recs.append([name, rng.integers(65, 91, l).astype(np.uint8).tobytes(), rng.integers(33, 127, l).astype(np.uint8).tobytes()])
        begin.append(b); end.append(e)
        size += len(name) + 2 * (e - b) + 6

    while size < (cap + 101) * tile:
        dense = size >= cap * tile                                  # the second round: more short records per tile
        add(int(rng.integers(2000, 4000 if dense else 9001)), b"read/%d" % len(recs))
        for l in rng.integers(0, 101, int(rng.integers(0, 16 if dense else 8))).tolist():
            add(l, bytes(rng.integers(48, 123, int(rng.integers(0, 41))).astype(np.uint8)))
        if len(recs) % 5 == 0:
            for _ in range(int(rng.integers(3, 9))):
                add(0, b"")
    add(50, b"last")
    add(0, b""); add(0, b"")
    if size % tile == 0:
        add(1, b"x")
    return recs, np.array(begin, dtype=np.uint32), np.array(end, dtype=np.uint32)


def check_format_past_cap(lib):
    tile, cap = LC.header_define("LQ_FASTQ_TILE"), LC.header_define("LQ_FASTQ_MAX_BLOCKS")
    t0 = time.time()
    recs, begin, end = caps_input(seed=202)
    n = len(recs)
    want = b"".join(b"@" + r[0] + b"\n" + r[1][b:e] + b"\n+\n" + r[2][b:e] + b"\n" for r, b, e in zip(recs, begin.tolist(), end.tolist()))
    total = len(want)
    n_tiles = (total + tile - 1) // tile
    LC.assert_past_cap("k_fastq_format, tiles", n_tiles, cap)
    assert total % tile != 0                                        # the last tile is partial
    assert n_tiles - cap < 110                                      # (the smallest such input)
    # the shape of the second round
    nl = np.array([len(r[0]) for r in recs], dtype=np.int64)
    lens = np.array([len(r[1]) for r in recs], dtype=np.int64)
    m = end.astype(np.int64) - begin.astype(np.int64)
    rec = np.concatenate([[0], np.cumsum(nl + 2 * m + 6)])
    assert rec[n] == total
    second = rec[:-1] >= cap * tile
    assert second.sum() >= 100
    seq_at, plus_at = rec[:-1] + nl + 2, rec[:-1] + nl + 2 + m + 1
    for at in (rec[:-1], seq_at, plus_at, plus_at + 2):             # record, bases, '+' and qualities begin at every residue
        assert set((at[second] % 16).tolist()) == set(range(16))
    for part in (second, ~second):
        bare = (part & (lens == 0) & (nl == 0)).astype(np.int8)
        assert (np.convolve(bare, np.ones(3, np.int8), "valid") == 3).sum() >= 3      # runs of empty reads without names
        assert (part & (lens >= 2000)).sum() >= 10 and (part & (lens > 0) & (lens <= 100)).sum() >= 50
    cut = (begin > 0) & (end < lens)
    assert cut.sum() >= 100 and (cut & second).sum() >= 10          # non-trivial bounds
    LC.timed("format input (%d reads, %d text bytes, %d tiles)" % (n, total, n_tiles), t0)
    t0 = time.time()
    ch = chunkpass.ReadChunk(recs, lib=lib)
    got = ch.fastq_bytes(begin, end)
    ch.close()
    LC.timed("ReadChunk + fastq_bytes", t0)
    if got != want:
        assert len(got) == total, "%d bytes of text instead of %d" % (len(got), total)
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(g != w)
        raise AssertionError("%d bytes differ, first at %s (the second round starts at byte %d): %s != %s" % (
            bad.shape[0], bad[:5], cap * tile, g[bad[:5]], w[bad[:5]]))


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_format_past_the_cap(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_format_past_cap(emu_lib)


@pytest.mark.gpu
def test_gpu_format_past_the_cap(gpu_lib):
    check_format_past_cap(gpu_lib)

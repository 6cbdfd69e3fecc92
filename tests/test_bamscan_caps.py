"""The k_bam_* kernels past their launch caps (kernels_bamscan.hpp), after the scheme of tests/test_fxscan_caps.py: the smallest BAM of tiny
records (l_seq 0..3) that makes every one of them run its grid-stride loop a second time in one scan -- more byte tiles than
k_bam_candidates has blocks, more candidate tiles than k_bam_link, k_fx_jump and k_bam_emit have, more tile counts than k_fx_tilescan's
one block has lanes, more segments than one round of k_fx_rebase moves -- and, with a few long reads behind them, more gather tiles
than one round of k_fx_tileseg names.  Caps and tiles are read from the headers.  The expected records are the list written; the
number of candidates the scan must report is counted in numpy from the cheap test."""
import struct
import time

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import bam_writer as BW
from tests import test_launch_caps as LC

CODE = np.zeros(256, np.uint8)
CODE[list(BW.CODES)] = np.arange(16)


def record(name, s, q):
    """bam_writer.record with numpy doing the packing (s: the bases as a uint8 array of letters, q: the quality bytes)"""
    l = s.shape[0]
    c = CODE[s]
    if l & 1:
        c = np.append(c, np.uint8(0))
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm), 0, 4680, 0, 4, l, -1, -1, 0) + nm + (c[0::2] << 4 | c[1::2]).tobytes() + q
    return struct.pack("<i", len(body)) + body


def caps_input(seed):
    """-> (the inflated bytes, names, sequences, qualities as chr(q + 33))"""
    rng = np.random.default_rng(seed)
    cap, ltile, threads = LC.header_define("LQ_FXSCAN_MAX_BLOCKS"), LC.header_define("LQ_FXSCAN_LINE_TILE"), LC.header_define("LQ_FXSCAN_THREADS")
    n_tiny = (cap + 101) * ltile + 17                               # with l_seq 0 every 16th: more segments than cap * threads as well
    want_bases = (LC.header_define("LQ_FXSCAN_TILESEG_MAX_BLOCKS") * threads + 101) * LC.header_define("LQ_GATHER_TILE")
    letters = np.frombuffer(BW.CODES, np.uint8)
    flat = letters[rng.integers(0, 16, 3 * n_tiny)]
    qflat = rng.integers(0, 94, 3 * n_tiny).astype(np.uint8)
    parts, names, seqs, quals = [BW.header()], [], [], []
    for i in range(n_tiny):
        l = 0 if i % 16 == 5 else 1 + i % 3
        s, q = flat[3 * i:3 * i + l], (qflat[3 * i:3 * i + l] if i % 7 else np.full(l, 255, np.uint8))
        names.append(b"t%d" % i); seqs.append(s.tobytes()); quals.append((q + 33).tobytes() if l and q[0] != 255 else b"!" * l)
        parts.append(record(names[-1], s, q.tobytes()))
    bases, i = sum(len(s) for s in seqs), 0
    while bases < want_bases:                                       # the gather's tiles: long reads, some without qualities
        l = int(rng.integers(700000, 900000))
        s, q = letters[rng.integers(0, 16, l)], (rng.integers(0, 94, l).astype(np.uint8) if i % 2 else np.full(l, 255, np.uint8))
        names.append(b"long%d" % i); seqs.append(s.tobytes()); quals.append((q + 33).tobytes() if q[0] != 255 else b"!" * l)
        parts.append(record(names[-1], s, q.tobytes()))
        bases += l; i += 1
    parts.append(record(b"last", letters[:5], bytes(range(5))))
    names.append(b"last"); seqs.append(BW.CODES[:5]); quals.append(bytes(range(33, 38)))
    return b"".join(parts), names, seqs, quals


def candidates(data, lo):
    """how many offsets above lo pass the cheap test, and the start itself"""
    a = np.frombuffer(data, np.uint8)
    n = a.shape[0]
    run = np.concatenate(([0], np.cumsum(a == 255)))
    ff8 = run[8:] - run[:-8] == 8                                   # ff8[p]: bytes p .. p + 7 are 0xff
    o = np.arange(lo + 1, n - 36 + 1)
    return 1 + int((ff8[o + 4] & ff8[o + 24] & (a[o + 23] < 128)).sum())


def check_walk_past_caps(lib, tmp_path, monkeypatch):
    cap, tile, ltile, threads = (LC.header_define(k) for k in ("LQ_FXSCAN_MAX_BLOCKS", "LQ_FXSCAN_TILE", "LQ_FXSCAN_LINE_TILE", "LQ_FXSCAN_THREADS"))
    tcap, gtile = LC.header_define("LQ_FXSCAN_TILESEG_MAX_BLOCKS"), LC.header_define("LQ_GATHER_TILE")
    t0 = time.time()
    data, names, seqs, quals = caps_input(seed=78)
    n, total = len(names), sum(len(s) for s in seqs)
    hdr = len(BW.header())
    n_cand, n_segs = candidates(data, hdr), sum(1 for s in seqs if s)
    assert n_cand >= n                                              # (every record behind the first is a candidate)
    byte_tiles, cand_tiles, gather_tiles = (len(data) - (hdr & ~15) + tile - 1) // tile, (n_cand + ltile - 1) // ltile, (total + gtile - 1) // gtile
    LC.assert_past_cap("k_bam_candidates, byte tiles", byte_tiles, cap)
    LC.assert_past_cap("k_bam_link / k_fx_jump / k_bam_emit, candidate tiles", cand_tiles, cap)
    LC.assert_past_cap("k_fx_tilescan, tile counts", min(byte_tiles, cand_tiles), threads)
    LC.assert_past_cap("k_fx_rebase, segments", n_segs, cap * threads)
    LC.assert_past_cap("k_fx_tileseg, gather tiles", gather_tiles + 1, tcap * threads)
    assert (len(data) - hdr) % tile != 0 and n_cand % ltile != 0 and total % gtile != 0      # partial last tiles
    assert cand_tiles - cap < 160                                   # (the smallest such input)
    assert max(len(s) for s in seqs[:-8]) <= 3
    LC.timed("walk input (%d records, %d candidates, %d bytes)" % (n, n_cand, len(data)), t0)
    t0 = time.time()
    path = str(tmp_path / "caps.bam")
    open(path, "wb").write(BW.bgzf(data, level=1))
    monkeypatch.setenv("LQREADER_PIECE_BYTES", str(len(data) + 65536))      # the whole file is one piece
    L = chunkpass._lib(lib)
    fc = chunkpass.FileChunks(path, chunk_size=1 << 40, lib=lib, is_sequel=False, bam_walk="device")
    got = []
    for ch, n_seqs, n_bases in fc:
        assert (ch.n, n_seqs, n_bases) == (n, n, total)
        assert ch.names == [x.decode() for x in names] and ch.lens.tolist() == [len(s) for s in seqs]
        g_seq, g_qual = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        assert L.lqchunk_get_reads(ch.h, 0, None, g_seq.ctypes.data, g_qual.ctypes.data) == 0
        got.append((g_seq.tobytes(), g_qual.tobytes()))
    LC.timed("FileChunks(bam_walk='device') + lqchunk_get_reads", t0)
    st = fc.parse_stats
    assert len(got) == 1 and st["scans"] == 1 and st["records_device"] == n and st["records_host"] == 0 and st["lines"] == n_cand, st      # one scan found them all
    assert got[0][0] == b"".join(seqs)
    assert got[0][1] == b"".join(quals)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_walk_past_the_caps(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_walk_past_caps(emu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_walk_past_the_caps(gpu_lib, tmp_path, monkeypatch):
    check_walk_past_caps(gpu_lib, tmp_path, monkeypatch)

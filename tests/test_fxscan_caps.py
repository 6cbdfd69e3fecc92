"""The k_fx_* kernels past their launch caps (kernels_fxscan.hpp), after the scheme of tests/test_filechunks_caps.py: the smallest seeded
file that makes every one of them run its loop a second time in one scan -- more byte tiles than k_fx_lines has blocks, more line
tiles than k_fx_candidates, k_fx_jump and k_fx_emit have, more tile counts than k_fx_tilescan's one block has lanes, more segments
than one round of k_fx_rebase moves and more gather tiles than one round of k_fx_tileseg names.  Caps and tiles are read from the
header.  The file is FASTA wrapped at 16 columns with a FASTQ record on one line after every tenth record, so wrapped and one-line
records fall into the second round; the reference is kseq_records."""
import time

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_filechunks as TF
from tests import test_launch_caps as LC

WIDTH = 16


def caps_input(seed):
    rng = np.random.default_rng(seed)
    cap, ltile, threads = LC.header_define("LQ_FXSCAN_MAX_BLOCKS"), LC.header_define("LQ_FXSCAN_LINE_TILE"), LC.header_define("LQ_FXSCAN_THREADS")
    want_lines = max((cap + 101) * ltile, cap * threads + 200)
    want_bases = (LC.header_define("LQ_FXSCAN_TILESEG_MAX_BLOCKS") * threads + 101) * LC.header_define("LQ_GATHER_TILE")
    parts, n_lines, bases, i = [], 0, 0, 0
    alphabet = np.frombuffer(b"ACGTacgtNn", np.uint8)
    while n_lines < want_lines or bases < want_bases:
        l = int(rng.integers(1500, 1700))
        bases += l
        seq = alphabet[rng.integers(0, alphabet.shape[0], l)].tobytes()
        parts.append(b">w%d c\n" % i + TF.wrap(seq, WIDTH, b"\n"))
        n_lines += 1 + (l + WIDTH - 1) // WIDTH
        if i % 10 == 9:
            l = int(rng.integers(0, 300))
            seq = alphabet[rng.integers(0, alphabet.shape[0], l)].tobytes()
            parts.append(b"@q%d\n" % i + seq + b"\n+\n" + rng.integers(33, 127, l).astype(np.uint8).tobytes() + b"\n")
            n_lines += 4
            bases += l
        i += 1
    parts.append(b"@last\nACGTA\n+\n@>+I!\n")
    return b"".join(parts)


def check_scan_past_caps(lib, tmp_path):
    cap, tile, ltile, threads = (LC.header_define(k) for k in ("LQ_FXSCAN_MAX_BLOCKS", "LQ_FXSCAN_TILE", "LQ_FXSCAN_LINE_TILE", "LQ_FXSCAN_THREADS"))
    tcap, gtile = LC.header_define("LQ_FXSCAN_TILESEG_MAX_BLOCKS"), LC.header_define("LQ_GATHER_TILE")
    t0 = time.time()
    data = caps_input(seed=77)
    records, src, dst = TF.kseq_records(data)
    n_lines = data.count(b"\n") + 1
    total = sum(len(r[1]) for r in records)
    n_sseg = sum(1 for r in records for _ in range(0, len(r[1]), WIDTH if r[2] is None else 1 << 30))
    byte_tiles, line_tiles, gather_tiles = (len(data) + tile - 1) // tile, (n_lines + ltile - 1) // ltile, (total + gtile - 1) // gtile
    LC.assert_past_cap("k_fx_lines, byte tiles", byte_tiles, cap)
    LC.assert_past_cap("k_fx_candidates / k_fx_jump / k_fx_emit, line tiles", line_tiles, cap)
    LC.assert_past_cap("k_fx_tilescan, tile counts", min(byte_tiles, line_tiles), threads)
    LC.assert_past_cap("k_fx_rebase, sequence segments", n_sseg, cap * threads)
    LC.assert_past_cap("k_fx_tileseg, gather tiles", gather_tiles + 1, tcap * threads)
    assert len(data) % tile != 0 and n_lines % ltile != 0 and len(data) % 16384 != 0        # partial last tiles
    assert line_tiles - cap < 160                                   # (the smallest such input)
    second = data[:0].join([data[cap * tile:]])                     # what the second round of k_fx_lines reads: wrapped and one-line records
    assert second.count(b"\n>w") >= 100 and second.count(b"\n@q") >= 10
    LC.timed("scan input (%d records, %d lines, %d bytes)" % (len(records), n_lines, len(data)), t0)
    t0 = time.time()
    path = str(tmp_path / "caps.fx")
    open(path, "wb").write(data)
    L = chunkpass._lib(lib)
    fc = chunkpass.FileChunks(path, chunk_size=1 << 40, is_upper=False, lib=lib, parse="device")
    got = []
    for ch, n_seqs, n_bases in fc:
        assert (ch.n, n_seqs, n_bases) == (len(records), len(records), total)
        assert ch.names == [r[0].split()[0].decode() for r in records] and ch.lens.tolist() == [len(r[1]) for r in records]
        g_seq, g_qual = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        assert L.lqchunk_get_reads(ch.h, 0, None, g_seq.ctypes.data, g_qual.ctypes.data) == 0
        got.append((g_seq.tobytes(), g_qual.tobytes()))
    LC.timed("FileChunks(parse='device') + lqchunk_get_reads", t0)
    st = fc.parse_stats
    assert len(got) == 1 and st["scans"] == 1 and st["records_device"] == len(records) and st["lines"] == n_lines, st      # one scan found them all
    assert got[0][0] == b"".join(r[1] for r in records)
    assert got[0][1] == b"".join(r[2] if r[2] is not None else b"!" * len(r[1]) for r in records)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_scan_past_the_caps(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_scan_past_caps(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_scan_past_the_caps(gpu_lib, tmp_path):
    check_scan_past_caps(gpu_lib, tmp_path)

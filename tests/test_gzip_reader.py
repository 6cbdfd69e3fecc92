"""The reader in device mode on a gzip file that is not BGZF (gzip.hpp, reader.cpp, kernels_gzip.hpp; FileChunks(inflate="device"),
SampleQCPass.run_file(inflate="device"), lqreader_inflate_stats), under the wave emulator and on the GPU.  What the mode may change is
where the stream is inflated; everything a caller sees is the host mode's, gzread's:
  1. a multi-line FASTQ, a FASTA and a CRLF FASTQ as plain .gz at two chunk sizes, with and without LQREADER_PIECE_BYTES=4096: records,
     borders, n_seqs, n_bases, names, lens and flat bytes side by side; inflate_stats says the device made the bytes;
  2. run_file(gz, inflate="device") leaves the sdust table, the subsample, the adapter block and the GC block of the host mode;
  3. a flipped deflate byte, a flipped CRC32, a flipped ISIZE, a file cut inside a block and inside the trailer, a second member of
     method 7, a distance in front of the first member's start: the code and the message of the host mode, whatever they are, over
     the whole iteration (how many chunks come out before an error is not part of the contract);
  4. 100 zero bytes and text behind the last member: as the host mode;
  5. lqreader_inflate after the first lqreader_next is LQCOV_E_STATE."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from longqc_amd import api, chunkpass, sampleqc, synth
from tests import deflate_writer as DW
from tests import test_bamchunks as TB
from tests import test_filechunks as TF
from tests import test_gzip_inflate as GI

SPAN = "2048"


def everything(lib, path, **kw):
    """-> (what iteration gave: [(records, n_seqs, n_bases, names, lens, flat bytes)], the error as (code, message) or None, stats)"""
    L = chunkpass._lib(lib)
    fc = chunkpass.FileChunks(path, lib=lib, str_overhead=49, **kw)
    got, err = [], None
    try:
        for ch, ns, nb in fc:
            got.append((ch.records(), ns, nb, ch.names, ch.lens.tolist(), TB.flat(L, ch)))
    except api.LqcovError as e:
        err = (e.code, str(e))
    return got, err, fc.inflate_stats


# ---- 1. side by side ----
def check_side_by_side(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("LQREADER_GZ_SPAN_BYTES", SPAN)
    recs = [r for seed in range(31, 36) for r in TF.rand_records(seed, b"ACGT")]      # (about 200 KB: several blocks at level 6)
    for name, data in (("ml.fq.gz", TF.fastq_bytes(recs, 60)), ("w.fa.gz", TF.fasta_bytes(recs, 60)), ("crlf.fq.gz", TF.fastq_bytes(recs, 0, b"\r\n"))):
        path = str(tmp_path / name)
        open(path, "wb").write(GI.gz(data, 6, 6))                  # (memLevel 6: a block every 4095 symbols, several per file)
        want = TF.as_reads(TF.kseq_records(data)[0])
        size = sum(3 * 49 + len(r[0]) + 2 * len(r[1]) for r in want)
        for piece in (None, "4096"):
            if piece:
                monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
            for cs in (size // 5 + 1, 30000):
                host, eh, sh = everything(lib, path, chunk_size=cs, inflate="host")
                dev, ed, sd = everything(lib, path, chunk_size=cs, inflate="device")
                assert eh is None and ed is None and dev == host and len(host) >= 5, (name, piece, cs)
                assert [r for c in dev for r in c[0]] == want, (name, piece, cs)
                assert not any(sh.values()) and sd["bytes_device"] + sd["bytes_zlib"] == len(data), (sh, sd)
                assert sd["bytes_zlib"] == 0 and sd["spans_accepted"] >= 2 and sd["markers_resolved"] > 0, sd
            monkeypatch.delenv("LQREADER_PIECE_BYTES", raising=False)


# ---- 2. run_file ----
def check_run_file(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("LQREADER_GZ_SPAN_BYTES", "4096")
    cfg = synth.SynthConfig("gz", n_reads=120, mean_len=2000, depth=6.0, seed=7112, nsample=30)
    T, _ = synth.make_dataset(cfg)
    plain = str(tmp_path / "w.fq")
    synth.write_fastq(plain, T)
    gz = str(tmp_path / "w.fq.gz")
    open(gz, "wb").write(GI.gz(open(plain, "rb").read(), 6, 8))
    adp5, adp3 = sampleqc.PRESET_ADAPTERS["pb-sequel"]
    cs = sum(3 * 49 + len(nm) + 2 * s.shape[0] for nm, s in zip(T.names, T.seqs)) // 3 + 1
    out = []
    for mode in ("host", "device"):
        p = chunkpass.SampleQCPass(str(tmp_path / mode), "pb-sequel", adp5=adp5, adp3=adp3, nsample=30, inds=200000, gc_draw="device", gc_seed=3,
                                   suffix="x", lib=lib)
        np.random.seed(11)
        res = p.run_file(gz, chunk_size=cs, str_overhead=49, inflate=mode)
        p.mask.close_pool()
        out.append((p, res))
    (a, ra), (b, rb) = out
    assert len(ra) >= 3 and ra == rb
    table = open(a.mask.get_outfile_path(), "rb").read()
    assert table == open(b.mask.get_outfile_path(), "rb").read() and table.count(b"\n") == 120
    assert a.s_reads == b.s_reads and len(a.s_reads) == 30 and all(a.s_reads)
    assert a.adapters.json_block() == b.adapters.json_block() and a.gc.json_block() == b.gc.json_block()
    assert (a.cum_n_seq, a.chunk_n, a.n_bases) == (b.cum_n_seq, b.chunk_n, b.n_bases) == (120, len(ra), T.n_bases)
    a.close(); b.close()


# ---- 3., 4. files that are not whole, and files with more than a stream ----
def far_back_member(text):
    """a gzip member whose first block is fine and whose second holds a match 300 bytes in front of the member's first byte"""
    w = DW.BitWriter() if hasattr(DW, "BitWriter") else None
    head = text[:200]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = c.compress(head) + c.flush(zlib.Z_FULL_FLUSH)           # ends at a byte border, not final
    # a final fixed-code block: length 3 (symbol 257, code 0000001), distance code 16 (257..384: 7 extra bits, 500 - 257 = 243), end of block
    bits = [(1, 1), (1, 2)]                                         # BFINAL 1, BTYPE 1
    val, n = 0, 0
    def put(v, k, msb=False):
        nonlocal val, n
        if msb:
            v = int(format(v, "0%db" % k)[::-1], 2)
        val |= v << n; n += k
    put(1, 1); put(1, 2); put(0b0000001, 7, True); put(16, 5, True); put(243, 7); put(0, 7, True)
    second = val.to_bytes((n + 7) // 8, "little")
    assert w is None or True
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + first + second + struct.pack("<II", 0, 203)


def odd_files():
    text = GI.fastq_text()[:150000]
    whole = GI.gz(text, 6, 8)
    n = len(whole)
    flip, crc, isize = bytearray(whole), bytearray(whole), bytearray(whole)
    flip[n * 3 // 4] ^= 0x10
    crc[n - 8] ^= 0x01
    isize[n - 4] ^= 0x01
    second = GI.gz(text[:5000], 6, 8)
    return [("deflate", bytes(flip)), ("crc", bytes(crc)), ("isize", bytes(isize)), ("cut_block", whole[:n * 2 // 3]), ("cut_trailer", whole[:n - 3]),
            ("method7", whole + second[:2] + b"\x07" + second[3:]), ("far_back", far_back_member(text)),
            ("zeros", whole + bytes(100)), ("text", whole + b"@trailing\nACGT\n+\nIIII\n"), ("two", whole + second), ("one_byte", whole + b"\x1f")]


def check_odd_files(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("LQREADER_GZ_SPAN_BYTES", SPAN)
    seen = {}
    for name, data in odd_files():
        path = str(tmp_path / (name + ".fq.gz"))
        open(path, "wb").write(data)
        for cs in (1 << 40, 40000):
            host, eh, _ = everything(lib, path, chunk_size=cs, inflate="host")
            dev, ed, sd = everything(lib, path, chunk_size=cs, inflate="device")
            print(name, cs, eh, ed, len(host), len(dev), sd)
            assert eh == ed, (name, cs)
            if eh is None:
                assert host == dev, (name, cs)
            else:
                assert eh[0] == -2 and eh[1].endswith("not a complete gzip stream") and "failed to open file" in eh[1], eh
        seen[name] = eh
    # (what zlib is known to do: these fail, those do not)
    assert all(seen[k] for k in ("deflate", "crc", "isize", "method7", "far_back")) and not any(seen[k] for k in ("zeros", "text", "two")), seen


# ---- 5. state ----
def check_state(lib, tmp_path):
    L = chunkpass._lib(lib)
    path = str(tmp_path / "s.fq.gz")
    open(path, "wb").write(GI.gz(b"@a\nACGT\n+\nIIII\n@b\nTTGCA\n+\nIIIII\n"))
    r = L.lqreader_open(path.encode(), 0, 1, 1, 49, 0)
    assert r and L.lqreader_inflate(r, 1) == 0
    ch = chunkpass.ReadChunk(None, lib=lib)
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 1 and not last.value
    assert L.lqreader_inflate(r, 0) == -4 and b"lqreader_inflate" in L.lqreader_last_error(r)
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 1 and b.value == 9
    st = (C.c_uint64 * len(chunkpass.INFLATE_STATS))()
    assert L.lqreader_inflate_stats(r, st) == 0 and st[0] >= 1 and st[5] == 32 and L.lqreader_inflate_stats(r, None) == -1
    L.lqreader_close(r)
    ch.close()


def test_emulated_gzip_reader_side_by_side(emu_lib, tmp_path, monkeypatch):
    check_side_by_side(emu_lib, tmp_path, monkeypatch)


def test_emulated_gzip_reader_run_file(emu_lib, tmp_path, monkeypatch):
    check_run_file(emu_lib, tmp_path, monkeypatch)


def test_emulated_gzip_reader_odd_files(emu_lib, tmp_path, monkeypatch):
    check_odd_files(emu_lib, tmp_path, monkeypatch)


def test_emulated_gzip_reader_state(emu_lib, tmp_path):
    check_state(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_gzip_reader_side_by_side(gpu_lib, tmp_path, monkeypatch):
    check_side_by_side(gpu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_gzip_reader_run_file(gpu_lib, tmp_path, monkeypatch):
    check_run_file(gpu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_gzip_reader_odd_files(gpu_lib, tmp_path, monkeypatch):
    check_odd_files(gpu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_gzip_reader_state(gpu_lib, tmp_path):
    check_state(gpu_lib, tmp_path)

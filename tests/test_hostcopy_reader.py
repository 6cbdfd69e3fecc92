"""FileChunks(inflate="device", parse="device", host_copy="needed") against host_copy="all" and against the host modes (lqreader_host_copy,
reader.cpp over kernels_crc32.hpp and k_fx_names), under the wave emulator and on the GPU: the same chunk borders, counts, names,
record bytes, parse_stats and inflate_stats for bgzip and gzip files, in pieces of 4096 bytes and of the default size, for both
string overheads; run_file; the errors a CRC32 alone can notice; the readers that ignore the mode; and copy_stats, which must show
that the inflated bytes did not come back."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from longqc_amd import api, chunkpass
from tests import bam_writer
from tests import test_bamchunks as TB
from tests import test_filechunks as TF
from tests import test_gzip_inflate as GI
from tests import test_launch_caps as LC

DEVICE = dict(inflate="device", parse="device")


def everything(lib, path, **kw):
    """-> (what iteration gave, the error as (code, message) or None, the FileChunks)"""
    L = chunkpass._lib(lib)
    fc = chunkpass.FileChunks(path, lib=lib, **kw)
    got, err = [], None
    try:
        for ch, ns, nb in fc:
            got.append((ch.n, ns, nb, list(ch.names), ch.lens.tolist(), ch.records(), TB.flat(L, ch)))
    except api.LqcovError as e:
        err = (e.code, str(e))
    return got, err, fc


def same(lib, path, active=1, **kw):
    """host_copy "needed" gives what "all" gives, and what the host modes give -> (the chunks, the "needed" FileChunks)"""
    host, eh, _ = everything(lib, path, inflate="host", parse="host", **kw)
    every, ea, fa = everything(lib, path, host_copy="all", **DEVICE, **kw)
    need, en, fn = everything(lib, path, host_copy="needed", **DEVICE, **kw)
    assert eh is None and ea is None and en is None, (path, kw, eh, ea, en)
    assert [c[:3] for c in need] == [c[:3] for c in every], (path, kw)
    assert need == every == host, (path, kw)
    assert fn.parse_stats == fa.parse_stats and fn.inflate_stats == fa.inflate_stats, (path, kw, fn.parse_stats, fa.parse_stats, fn.inflate_stats, fa.inflate_stats)
    assert fa.copy_stats["active"] == 0 and fn.copy_stats["active"] == active, (fa.copy_stats, fn.copy_stats)
    assert fn.copy_stats["bytes_inflated"] == fa.copy_stats["bytes_inflated"]
    return need, fn


def short_records(n, seed):
    """FASTQ records of at most 256 bytes of text"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        l = int(rng.integers(1, 106))
        recs.append([b"r%d" % i + (b" len=%d" % l if i % 3 == 0 else b""), bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), l)),
                     bytes(rng.integers(33, 127, l).astype(np.uint8))])
    return recs


def mixed_member(data):
    """one gzip member whose deflate stream has a stored block, a fixed-code block and dynamic blocks"""
    a, b = len(data) // 5, len(data) // 3
    parts = []
    for piece, level, strategy, last in ((data[:a], 0, zlib.Z_DEFAULT_STRATEGY, False), (data[a:b], 6, zlib.Z_FIXED, False), (data[b:], 6, zlib.Z_DEFAULT_STRATEGY, True)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        parts.append(c.compress(piece) + c.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH))
    raw = b"".join(parts)
    assert zlib.decompress(raw, -15) == data
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def files(tmp_path):
    """name -> path; written once per directory"""
    recs = short_records(600, 21)
    long_recs = [r for seed in range(31, 33) for r in TF.rand_records(seed, b"ACGT")]
    text = TF.fastq_bytes(long_recs, 60)
    # a block that inflates to more than a span's region, even the doubled one: zlib's on the host, with the window from the device
    long_run = TF.fastq_bytes([[b"run", text[1000:1040].replace(b"\n", b"A") + b"A" * 400000, text[2000:2040].replace(b"\n", b"I") + b"I" * 400000]])
    made = {
        "short.bgz.fq.gz": bam_writer.bgzf(TF.fastq_bytes(recs), block_payload=1000),
        "w60.bgz.fa.gz": bam_writer.bgzf(TF.fasta_bytes(long_recs, 60), block_payload=900, empty_block_every=7),
        "crlf.bgz.fq.gz": bam_writer.bgzf(TF.fastq_bytes(long_recs, 0, b"\r\n"), block_payload=777, level=1),
        "one.fq.gz": GI.gz(text, 6, 6),
        "three.fq.gz": GI.gz(text[:30000], 6, 6) + GI.gz(text[30000:31000], 1, 8) + GI.gz(text[31000:], 6, 6),
        "mixed.fq.gz": mixed_member(text),
        "longrun.fq.gz": GI.gz(text[:40000] + long_run + text[40000:90000], 6, 8),
        "empty.bgz.fq.gz": bam_writer.bgzf(b""),
        "empty.fq.gz": GI.gz(b""),
        "single.bgz.fq.gz": bam_writer.bgzf(b"@only one\nACGTACGT\n+\nIIIIIIII\n"),
        "single.fq.gz": GI.gz(b"@only one\nACGTACGT\n+\nIIIIIIII\n"),
    }
    out = {}
    for name, data in made.items():
        out[name] = str(tmp_path / name)
        open(out[name], "wb").write(data)
    return out, recs


def check_parity(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("LQREADER_GZ_SPAN_BYTES", "2048")
    paths, _ = files(tmp_path)
    for piece, shapes in (("4096", ((49, 2000), (41, 30000))), (None, ((49, 1 << 30),))):      # (2000: chunks end inside a piece's vouched records)
        if piece:
            monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
        else:
            monkeypatch.delenv("LQREADER_PIECE_BYTES")
        for name, path in paths.items():
            for ov, cs in shapes:
                got, fn = same(lib, path, str_overhead=ov, chunk_size=cs)
            st = fn.copy_stats
            if name.startswith(("empty", "single")):
                continue
            assert st["names_device"] == fn.parse_stats["records_device"] > 0, (name, st, fn.parse_stats)
            assert st["bytes_crc_device"] + st["bytes_crc_host"] == st["bytes_inflated"] > 0, (name, st)
            # zlib's bytes are checked where they are made.  (The span kernels decode stored and fixed-code blocks themselves, so
            # mixed.fq.gz needs no zlib; the block of longrun.fq.gz that fits no region does.)
            assert (st["bytes_crc_host"] > 0) == (name == "longrun.fq.gz"), (name, st)
            assert st["bytes_crc_host"] == fn.inflate_stats["bytes_zlib"], (name, st, fn.inflate_stats)


def check_copy_stats(lib, tmp_path, monkeypatch):
    """the clean bgzip FASTQ, records of at most 256 bytes of text, pieces of 4096: per piece only the bytes behind the last vouched
    record come back, less than two records of 4096 bytes"""
    monkeypatch.setenv("LQREADER_PIECE_BYTES", "4096")
    paths, recs = files(tmp_path)
    assert max(len(TF.fastq_bytes([r])) for r in recs) <= 256
    got, fn = same(lib, paths["short.bgz.fq.gz"], str_overhead=49, chunk_size=50000)
    st, ps = fn.copy_stats, fn.parse_stats
    print(st, ps)
    assert got[-1][1] == len(recs) and len(got) >= 3
    assert st["active"] == 1
    assert st["bytes_inflated"] == len(TF.fastq_bytes(recs))
    assert st["bytes_crc_device"] == st["bytes_inflated"]
    assert st["bytes_crc_host"] == 0
    assert st["names_device"] == ps["records_device"]
    assert st["bytes_to_host"] <= st["bytes_inflated"] // 4


def check_run_file(lib, tmp_path):
    from longqc_amd import synth
    T, _ = synth.make_dataset(synth.CONFIGS["tiny"])
    plain = str(tmp_path / "tiny.fq")
    synth.write_fastq(plain, T)
    path = str(tmp_path / "tiny.bgz.fq.gz")
    open(path, "wb").write(bam_writer.bgzf(open(plain, "rb").read(), block_payload=20000))
    kw = dict(adp5=TF.ADP5, adp3=TF.ADP3, nsample=20, inds=100000, gc_draw="device", gc_seed=3, suffix="x", lib=lib)
    out = []
    for tag, mode in (("a", "all"), ("n", "needed")):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "ont-ligation", **kw)
        np.random.seed(11)
        res = p.run_file(path, chunk_size=150000, str_overhead=49, host_copy=mode, **DEVICE)
        p.mask.close_pool()
        out.append((res, open(p.mask.get_outfile_path(), "rb").read(), p.s_reads, p.gc.json_block(), p.adapters.json_block(), (p.cum_n_seq, p.chunk_n, p.n_bases)))
        p.close()
    assert out[0] == out[1] and len(out[0][0]) >= 3 and out[0][1].count(b"\n") == len(T)


def check_errors(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("LQREADER_GZ_SPAN_BYTES", "2048")
    recs = short_records(300, 5)
    text = TF.fastq_bytes(recs)
    blocks = [bam_writer.bgzf_block(text[i:i + 1000], level=0 if k == 4 else 6) for k, i in enumerate(range(0, len(text), 1000))]
    eof = bam_writer.bgzf(b"")

    def joined(change):
        b = [bytearray(x) for x in blocks]
        change(b)
        return b"".join(bytes(x) for x in b) + eof

    def crc_field(b):
        b[7][-8] ^= 0x40

    def stored_payload(b):                                          # (the deflate stream stays valid: only the CRC32 can notice)
        b[4][18 + 5 + 300] ^= 0x01

    def two(b):
        b[9][-7] ^= 0x01; b[3][-5] ^= 0x80

    gz = bytearray(GI.gz(text, 6, 6))
    gz[-8] ^= 0x01
    bad_name = TF.fastq_bytes(recs[:100] + [[b"caf\x80", b"ACGT", b"IIII"]] + recs[100:])
    cases = [("crc.bgz.fq.gz", joined(crc_field), -2, "CRC32 mismatch", sum(map(len, blocks[:7]))),
             ("stored.bgz.fq.gz", joined(stored_payload), -2, "CRC32 mismatch", sum(map(len, blocks[:4]))),
             ("two.bgz.fq.gz", joined(two), -2, "CRC32 mismatch", sum(map(len, blocks[:3]))),
             ("trailer.fq.gz", bytes(gz), -2, "not a complete gzip stream", None),
             ("name.bgz.fq.gz", bam_writer.bgzf(bad_name, block_payload=1000), -5, "(read 101)", None),
             ("name.fq.gz", GI.gz(bad_name, 6, 6), -5, "(read 101)", None)]
    for piece in ("4096", None):
        if piece:
            monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
        else:
            monkeypatch.delenv("LQREADER_PIECE_BYTES")
        for name, data, code, text_part, at in cases:
            path = str(tmp_path / name)
            open(path, "wb").write(data)
            for cs in (1 << 30, 20000):
                every, ea, _ = everything(lib, path, host_copy="all", chunk_size=cs, **DEVICE)
                need, en, fn = everything(lib, path, host_copy="needed", chunk_size=cs, **DEVICE)
                _, eh, _ = everything(lib, path, inflate="host", parse="host", chunk_size=cs)
                assert en is not None and en == ea, (name, piece, cs, en, ea)
                assert en[0] == code and text_part in en[1], (name, en)
                assert at is None or "file offset %d:" % at in en[1], (name, en)
                assert eh is not None and eh[0] == code, (name, eh)
                if code == -5:                                      # the records in front of the name have joined
                    assert need == every and en == eh, (name, piece, cs)
                assert fn.copy_stats["active"] == 1


def check_ignored(lib, tmp_path):
    reads = [(b"b%d" % i, bytes(np.random.default_rng(i).choice(np.frombuffer(b"ACGT", np.uint8), 50 + 7 * i))) for i in range(40)]
    bam = str(tmp_path / "x.bam")
    bam_writer.write_bam(bam, reads, block_payload=700)
    text = TF.fastq_bytes(short_records(200, 9))
    plain, bg = str(tmp_path / "plain.fq"), str(tmp_path / "p.bgz.fq.gz")
    open(plain, "wb").write(text)
    open(bg, "wb").write(bam_writer.bgzf(text, block_payload=1000))
    for path, kw in ((bam, DEVICE), (plain, DEVICE), (bg, dict(inflate="device", parse="host")), (bg, dict(inflate="host", parse="device"))):
        every, ea, fa = everything(lib, path, host_copy="all", chunk_size=3000, **kw)
        need, en, fn = everything(lib, path, host_copy="needed", chunk_size=3000, **kw)
        assert ea is None and en is None and need == every and len(need) >= 2, (path, kw)
        assert fn.copy_stats["active"] == 0 and fn.copy_stats == fa.copy_stats, (path, kw, fn.copy_stats, fa.copy_stats)
        assert fn.parse_stats == fa.parse_stats and fn.copy_stats["names_device"] == 0 and fn.copy_stats["bytes_crc_device"] == 0


def check_state(lib, tmp_path, monkeypatch):
    L = chunkpass._lib(lib)
    path = str(tmp_path / "s.bgz.fq.gz")
    open(path, "wb").write(bam_writer.bgzf(b"@a\nACGT\n+\nIIII\n@b\nTTGCA\n+\nIIIII\n"))
    r = L.lqreader_open(path.encode(), 0, 1, 1, 49, 0)
    assert r and L.lqreader_inflate(r, 1) == 0 and L.lqreader_parse(r, 1) == 0
    assert L.lqreader_host_copy(r, 2) == -1 and L.lqreader_host_copy(None, 1) == -1
    assert L.lqreader_host_copy(r, 1) == 0 and L.lqreader_host_copy(r, 0) == 0 and L.lqreader_host_copy(r, 1) == 0
    ch = chunkpass.ReadChunk(None, lib=lib)
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 1 and not last.value
    assert L.lqreader_host_copy(r, 0) == -4 and b"lqreader_host_copy" in L.lqreader_last_error(r)
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 1 and b.value == 9
    st = (C.c_uint64 * len(chunkpass.COPY_STATS))()
    assert L.lqreader_copy_stats(r, st) == 0 and st[0] == 1 and st[1] == 32 and st[3] == 32 and L.lqreader_copy_stats(r, None) == -1
    L.lqreader_close(r)
    ch.close()
    # the environment applies where nothing is set
    monkeypatch.setenv("LQREADER_HOSTCOPY", "needed")
    assert chunkpass.host_copy_mode(None) == "needed" and chunkpass.host_copy_mode("all") == "all"
    _, err, fc = everything(lib, path, **DEVICE)
    assert err is None and fc.copy_stats["active"] == 1
    r = L.lqreader_open(path.encode(), 0, 1 << 30, 1, 49, 0)
    assert L.lqreader_inflate(r, 1) == 0 and L.lqreader_parse(r, 1) == 0
    ch = chunkpass.ReadChunk(None, lib=lib)
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 2
    assert L.lqreader_copy_stats(r, st) == 0 and st[0] == 1
    L.lqreader_close(r)
    ch.close()
    with pytest.raises(ValueError):
        chunkpass.FileChunks(path, lib=lib, host_copy="some")


CHECKS = [check_parity, check_copy_stats, check_run_file, check_errors, check_ignored, check_state]


def run(check, lib, tmp_path, monkeypatch):
    names = check.__code__.co_varnames[:check.__code__.co_argcount]
    check(*[dict(lib=lib, tmp_path=tmp_path, monkeypatch=monkeypatch)[k] for k in names])


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_emulated_host_copy_needed(emu_lib, tmp_path, monkeypatch, check):
    run(check, emu_lib, tmp_path, monkeypatch)


@pytest.mark.parametrize("order", LC.ORDERS[1:])
def test_emulated_host_copy_needed_thread_orders(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    run(check_copy_stats, emu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_gpu_host_copy_needed(gpu_lib, tmp_path, monkeypatch, check):
    run(check, gpu_lib, tmp_path, monkeypatch)

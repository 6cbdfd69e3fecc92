"""FileChunks(bam_walk="device") against the host walk of the same BAM (lqreader_bam_walk, reader.cpp over bamscan.hpp and
kernels_bamscan.hpp), under the wave emulator and on the GPU: the same chunk borders, counts, names, lengths and record bytes in pieces
of 64 and 4096 bytes and of the default size, for a header longer than a piece, both quality modes, both string overheads, chunks
that end inside a scan's rows, inflate on the host and on the device, and host_copy="needed", which a BAM honours exactly when the
device both inflates and walks it; parse_stats and copy_stats, which must show who found the records and that the inflated bytes did
not come back; one aligned record in the middle; the errors, by code and message; run_file; the switch's states.  With the switch
absent none of this can pass: records_device > 0 and active == 1 on a BAM are what the switch adds."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import bam_writer as BW
from tests import test_bamchunks as TB
from tests import test_filechunks as TF
from tests import test_hostcopy_reader as TH
from tests import test_launch_caps as LC

everything = TH.everything


def short_reads(n, seed):
    """reads whose records stay under 256 bytes: -> reads, quals, tags"""
    rng = random.Random(seed)
    reads, quals, tags = [], [], []
    for i in range(n):
        l = rng.randint(0, 100)
        reads.append([b"m%d/%d" % (i, l), bytes(rng.choice(BW.CODES) for _ in range(l))])
        quals.append(None if i % 5 == 2 else bytes(rng.randint(0, 93) for _ in range(l)))
        tags.append(bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 7, 30)))))
    return reads, quals, tags


def walks(lib, path, n_records=None, needed=True, **kw):
    """the device walk gives what the host walk gives, whoever inflates -> (the chunks, the FileChunks of the last device walk)"""
    host, eh, fh = everything(lib, path, **kw)
    assert eh is None and fh.parse_stats["scans"] == 0 and fh.copy_stats["active"] == 0, (path, kw, eh)
    modes = [dict(inflate="host"), dict(inflate="device"), dict(inflate="host", host_copy="needed")]
    if needed:
        modes.append(dict(inflate="device", host_copy="needed"))
    for mode in modes:
        got, e, fc = everything(lib, path, bam_walk="device", **mode, **kw)
        assert e is None, (path, kw, mode, e)
        assert [c[:3] for c in got] == [c[:3] for c in host], (path, kw, mode)
        assert got == host, (path, kw, mode)
        ps, cs = fc.parse_stats, fc.copy_stats
        active = int(mode == dict(inflate="device", host_copy="needed"))
        assert cs["active"] == active, (mode, cs)
        if n_records is not None:                                   # a clean file
            assert ps["records_device"] + ps["records_host"] == n_records, (mode, ps)
            assert ps["records_host"] <= ps["pieces"] + 1 and ps["fallbacks"] == 0, (mode, ps)
            assert n_records < 3 or ps["records_device"] > 0, (mode, ps)
        if active:
            assert cs["bytes_crc_host"] == 0 and cs["bytes_crc_device"] == cs["bytes_inflated"] > 0, cs
            assert cs["names_device"] == ps["records_device"], (cs, ps)
        else:
            assert cs["names_device"] == 0 and cs["bytes_crc_device"] == 0, cs
    return host, fc


def set_piece(monkeypatch, piece):
    if piece:
        monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
    else:
        monkeypatch.delenv("LQREADER_PIECE_BYTES", raising=False)


def check_parity(lib, tmp_path, monkeypatch):
    reads, cigars, tags, flags = TB.seeded_reads()
    rng = random.Random(6)
    quals = [None if i % 4 == 1 else bytes(rng.randint(0, 93) for _ in r[1]) for i, r in enumerate(reads)]
    plain, refs = str(tmp_path / "p.bam"), str(tmp_path / "refs.bam")
    BW.write_bam(plain, reads, quals, 4096, 6, TB.HEADER_TEXT, (), cigars, tags, flags)
    # a header with references that is longer than a piece of 4096 bytes
    stream = BW.write_bam(refs, reads, quals, 777, 6, b"@CO\t" + b"x" * 9000 + b"\n", [(b"chr%d" % i, 1000 + i) for i in range(30)], cigars, tags, flags,
                          empty_block_every=5)
    assert len(stream) - sum(len(BW.record(r[0], r[1], q, c, t, f)) for r, q, c, t, f in zip(reads, quals, cigars, tags, flags)) > 2 * 4096
    size = sum(3 * 49 + len(r[0]) + 2 * len(r[1]) for r in reads)
    for piece in ("64", "4096", None):                              # (64: shorter than a record's fixed part and name)
        set_piece(monkeypatch, piece)
        for path in (plain, refs):
            for sequel, ov, cs in ((True, 49, 1 << 30), (False, 41, 2000), (False, 49, size // 4 + 1)):      # (2000: chunks end inside a scan's rows)
                host, fc = walks(lib, path, len(reads), chunk_size=cs, str_overhead=ov, is_sequel=sequel)
                assert host[-1][1] == len(reads) and (cs == 1 << 30 or len(host) >= 4)
                if piece is None and cs == 2000:
                    assert fc.parse_stats["scans"] < len(host)      # (a scan's rows served more than one chunk)
    set_piece(monkeypatch, None)
    empty = str(tmp_path / "empty.bam")
    BW.write_bam(empty, [])
    walks(lib, empty, 0)
    one = str(tmp_path / "one.bam")
    BW.write_bam(one, [(b"a", b"ACGT")])
    host, _ = walks(lib, one, 1)
    assert host[0][5] == [["a", "ACGT", "!!!!"]]


def check_copy_stats(lib, tmp_path, monkeypatch):
    """2100 records under 256 bytes in pieces of 4096: the host walk needs the header's piece once and less than one record per piece
    after that -- at most 4096 + 256 * pieces bytes, which the input's own sizes put under a quarter of the inflated bytes"""
    set_piece(monkeypatch, "4096")
    reads, quals, tags = short_reads(2100, 17)
    path = str(tmp_path / "short.bam")
    stream = BW.write_bam(path, reads, quals, 1000, 6, tags=tags)
    longest = max(len(BW.record(r[0], r[1], q, (), t)) for r, q, t in zip(reads, quals, tags))
    assert len(reads) >= 2000 and longest < 256 and len(BW.header()) < 4096
    pieces_bound = len(stream) // (4096 - 1000) + 2                 # (a piece takes whole blocks of 1000 bytes: at least 3096 new bytes)
    assert 4096 + 256 * pieces_bound <= len(stream) // 4
    host, fc = walks(lib, path, len(reads), chunk_size=50000, str_overhead=49, is_sequel=False)
    cs, ps = fc.copy_stats, fc.parse_stats
    print(cs, ps)
    assert host[-1][1] == len(reads) and len(host) >= 3
    assert cs["active"] == 1 and cs["bytes_inflated"] == len(stream) and cs["bytes_crc_host"] == 0 and cs["names_device"] > 0
    assert cs["bytes_to_host"] <= cs["bytes_inflated"] // 4, cs


def check_aligned_record(lib, tmp_path, monkeypatch):
    reads, quals, tags = short_reads(300, 23)
    stream = bytearray(BW.bam_stream(reads, quals, tags=tags))
    at = len(BW.header()) + sum(len(BW.record(r[0], r[1], q, (), t)) for r, q, t in list(zip(reads, quals, tags))[:150])
    assert stream[at + 4:at + 12] == b"\xff" * 8
    stream[at + 4:at + 12] = struct.pack("<ii", 0, 12345)            # refID 0, pos 12345: record 151 is aligned
    path = str(tmp_path / "aligned.bam")
    open(path, "wb").write(BW.bgzf(bytes(stream), 3000))
    for piece in ("4096", None):
        set_piece(monkeypatch, piece)
        host, eh, _ = everything(lib, path, chunk_size=20000)
        for mode in (dict(inflate="host"), dict(inflate="device", host_copy="needed")):
            got, e, fc = everything(lib, path, chunk_size=20000, bam_walk="device", **mode)
            ps = fc.parse_stats
            assert eh is None and e is None and got == host and host[-1][1] == 300 and len(host) >= 2, (piece, mode)
            assert ps["records_host"] >= 1 and ps["records_device"] >= 290 and ps["records_device"] + ps["records_host"] == 300, ps


def check_errors(lib, tmp_path, monkeypatch):
    """the cases of tests/test_bamchunks.py::check_errors: the device walk reports what the host walk reports"""
    reads = [[b"r%d" % i, b"ACGTNACGTN" * (3 + i)] for i in range(40)]
    stream = BW.bam_stream(reads)
    whole = BW.bgzf(stream, 300)
    blocks, at = [], 0
    while at < len(whole):
        blocks.append(at)
        at += struct.unpack_from("<H", whole, at + 16)[0] + 1
    rec1 = len(BW.header()) + len(BW.record(*reads[0]))

    def damaged(**kw):
        s = bytearray(stream)
        if "block_size" in kw:
            s[rec1:rec1 + 4] = struct.pack("<i", kw["block_size"])
        if "name" in kw:
            s[rec1 + 36:rec1 + 36 + len(kw["name"])] = kw["name"]
        if "l_name" in kw:
            s[rec1 + 12] = kw["l_name"]
        if "l_seq" in kw:
            s[rec1 + 20:rec1 + 24] = struct.pack("<I", kw["l_seq"])
        return BW.bgzf(bytes(s), 300)

    flipped = bytearray(whole)
    flipped[blocks[3] + 18 + 5] ^= 0x40
    rec20 = len(BW.header()) + sum(len(BW.record(*r)) for r in reads[:20])
    late = bytearray(stream)
    late[rec20:rec20 + 4] = struct.pack("<i", 40)
    cases = [("cut_in_block", whole[:blocks[5] + 40], -2, "cut short"),
             ("cut_between_blocks", whole[:blocks[5]], -2, "ends inside a record"),
             ("crc", bytes(flipped), -2, None),
             ("block_size", damaged(block_size=40), -2, "BAM record 2: block_size 40 is too small"),
             ("late_block_size", BW.bgzf(bytes(late), 300), -2, "BAM record 21: block_size 40 is too small"),
             ("l_name", damaged(l_name=0), -2, "BAM record 2: l_read_name is 0"),
             ("l_seq", damaged(l_seq=1 << 31), -5, "2^31-1"),
             ("no_nul", damaged(name=b"r1x"), -2, "BAM record 2: the read name has no NUL"),
             ("high_byte", damaged(name=b"\xc3\xa9"), -5, "(read 2)")]
    for piece in ("4096", None):
        set_piece(monkeypatch, piece)
        for name, data, code, text in cases:
            path = str(tmp_path / (name + ".bam"))
            open(path, "wb").write(data)
            for cs in ((1 << 30, 3000) if piece else (3000,)):
                for inflate, extra in (("host", {}), ("device", dict(host_copy="needed"))):
                    host, eh, _ = everything(lib, path, chunk_size=cs, inflate=inflate)
                    got, e, fc = everything(lib, path, chunk_size=cs, inflate=inflate, bam_walk="device", **extra)
                    assert eh is not None and e == eh, (name, piece, cs, inflate, extra, e, eh)
                    assert e[0] == code and (text is None or text in e[1]), (name, e)
                    assert got == host, (name, piece, cs, inflate, extra)
                    assert fc.copy_stats["active"] == int(bool(extra))
            if name == "late_block_size":
                assert fc.parse_stats["records_device"] >= 19, fc.parse_stats


def check_run_file(lib, tmp_path):
    from longqc_amd import synth
    T, _ = synth.make_dataset(synth.CONFIGS["tiny"])
    path = str(tmp_path / "tiny.bam")
    BW.write_bam(path, [(nm.encode(), s.tobytes()) for nm, s in zip(T.names, T.seqs)], [bytes((q - 33).tolist()) for q in T.quals], 20000, 6)
    kw = dict(adp5=TF.ADP5, adp3=TF.ADP3, nsample=20, inds=100000, gc_draw="device", gc_seed=3, suffix="x", lib=lib)
    out = []
    for tag, mode in (("h", {}), ("d", dict(bam_walk="device")), ("n", dict(bam_walk="device", inflate="device", host_copy="needed"))):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "ont-ligation", **kw)
        np.random.seed(11)
        res = p.run_file(path, chunk_size=150000, str_overhead=49, is_sequel=False, **mode)
        p.mask.close_pool()
        out.append((res, open(p.mask.get_outfile_path(), "rb").read(), p.s_reads, p.gc.json_block(), p.adapters.json_block(), (p.cum_n_seq, p.chunk_n, p.n_bases)))
        p.close()
    assert out[0] == out[1] == out[2] and len(out[0][0]) >= 3 and out[0][1].count(b"\n") == len(T)


def check_state(lib, tmp_path, monkeypatch):
    L = chunkpass._lib(lib)
    path = str(tmp_path / "s.bam")
    BW.write_bam(path, [(b"a", b"ACGT"), (b"b", b"TTGCA")])
    r = L.lqreader_open(path.encode(), 0, 1, 1, 49, 0)
    assert r and L.lqreader_format(r) == 1
    assert L.lqreader_bam_walk(r, 2) == -1 and L.lqreader_bam_walk(None, 1) == -1
    assert L.lqreader_bam_walk(r, 1) == 0 and L.lqreader_bam_walk(r, 0) == 0 and L.lqreader_bam_walk(r, 1) == 0
    ch = chunkpass.ReadChunk(None, lib=lib)
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 1 and not last.value
    assert L.lqreader_bam_walk(r, 0) == -4 and b"lqreader_bam_walk" in L.lqreader_last_error(r)
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 1 and b.value == 9
    st = (C.c_uint64 * len(chunkpass.PARSE_STATS))()
    assert L.lqreader_parse_stats(r, st) == 0 and st[2] + st[3] == 2 and st[2] >= 1 and st[1] >= 1
    L.lqreader_close(r)
    ch.close()
    # the default is the host walk, whatever lqreader_parse says; the environment applies where nothing is set
    _, err, fc = everything(lib, path, parse="device", inflate="device", host_copy="needed")
    assert err is None and fc.parse_stats["scans"] == 0 and fc.copy_stats["active"] == 0 and fc.bam_walk == "host"
    monkeypatch.setenv("LQREADER_BAMWALK", "device")
    assert chunkpass.bam_walk_mode(None) == "device" and chunkpass.bam_walk_mode("host") == "host"
    got, err, fc = everything(lib, path, inflate="device", host_copy="needed")
    assert err is None and fc.parse_stats["records_device"] > 0 and fc.copy_stats["active"] == 1 and got[-1][1] == 2
    r = L.lqreader_open(path.encode(), 0, 1 << 30, 1, 49, 0)       # (the library reads the variable itself)
    ch = chunkpass.ReadChunk(None, lib=lib)
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 2
    assert L.lqreader_parse_stats(r, st) == 0 and st[1] >= 1 and st[2] >= 1
    L.lqreader_close(r)
    ch.close()
    _, err, fc = everything(lib, path, bam_walk="host")
    assert err is None and fc.parse_stats["scans"] == 0
    monkeypatch.delenv("LQREADER_BAMWALK")
    with pytest.raises(ValueError):
        chunkpass.FileChunks(path, lib=lib, bam_walk="gpu")
    # a FASTA/FASTQ reader accepts the switch and ignores it
    fq = str(tmp_path / "p.fq")
    open(fq, "wb").write(b"@a\nACGT\n+\nIIII\n@b\nTTGCA\n+\nIIIII\n")
    got, err, fc = everything(lib, fq, bam_walk="device", host_copy="needed")
    assert err is None and got[-1][1] == 2 and fc.parse_stats["scans"] == 0 and fc.copy_stats["active"] == 0


CHECKS = [check_parity, check_copy_stats, check_aligned_record, check_errors, check_run_file, check_state]


def run(check, lib, tmp_path, monkeypatch):
    names = check.__code__.co_varnames[:check.__code__.co_argcount]
    check(*[dict(lib=lib, tmp_path=tmp_path, monkeypatch=monkeypatch)[k] for k in names])


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_emulated_bam_walk_device(emu_lib, tmp_path, monkeypatch, check):
    run(check, emu_lib, tmp_path, monkeypatch)


@pytest.mark.parametrize("order", LC.ORDERS[1:])
def test_emulated_bam_walk_device_thread_orders(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    run(check_copy_stats, emu_lib, tmp_path, monkeypatch)
    run(check_aligned_record, emu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_gpu_bam_walk_device(gpu_lib, tmp_path, monkeypatch, check):
    run(check, gpu_lib, tmp_path, monkeypatch)

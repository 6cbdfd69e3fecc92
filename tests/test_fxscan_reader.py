"""FileChunks(parse="device") against FileChunks(parse="host") (lqreader_parse, reader.cpp over fxscan.hpp / kernels_fxscan.hpp), under the
wave emulator and on the GPU: the same chunk borders, counts, names, lengths and record bytes for the golden files and the seeded
layouts of tests/test_filechunks.py, plain and gzipped, in pieces shorter than a record and longer than the file, for both string
overheads and a chunk size that cuts inside a piece; together with inflate="device"; run_file; the reader's errors; a BAM file.
parse_stats must show that the device, not the host parser, found the records of a clean file."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from longqc_amd import api, chunkpass
from tests import bam_writer
from tests import test_filechunks as TF
from tests import test_launch_caps as LC
from tests.conftest import GOLDEN


def chunks(lib, path, **kw):
    fc = chunkpass.FileChunks(path, lib=lib, **kw)
    out = [(ch.n, ns, nb, list(ch.names), ch.lens.tolist(), ch.records()) for ch, ns, nb in fc]
    return out, fc


def same(lib, path, **kw):
    want, _ = chunks(lib, path, parse="host", **kw)
    got, fc = chunks(lib, path, parse="device", **kw)
    assert [c[:3] for c in got] == [c[:3] for c in want], (path, kw)
    assert got == want, (path, kw)
    return got, fc.parse_stats


def check_parity(lib, tmp_path, monkeypatch):
    for fn in ("tiny_all.fq.gz", "adv_all.fa.gz", "adv_sub.fq.gz", "adv_sub.fa.gz"):
        got, st = same(lib, os.path.join(GOLDEN, fn))
        assert st["records_device"] >= got[-1][1] - 1 > 0
        same(lib, os.path.join(GOLDEN, fn), chunk_size=20000, str_overhead=41)
    files = TF.seeded_files()
    for name, data in files.items():
        plain, gz = str(tmp_path / name), str(tmp_path / (name + ".gz"))
        open(plain, "wb").write(data)
        with gzip.open(gz, "wb") as f:
            f.write(data)
        n = len(TF.kseq_records(data)[0])
        for path in (plain, gz):
            got, st = same(lib, path)
            assert got[-1][1] == n and st["records_device"] + st["records_host"] == n and st["scans"] >= 1
        same(lib, plain, is_upper=False, chunk_size=3000, str_overhead=41)
    for piece in ("64", "4096"):                                    # pieces shorter than a record, a record that doubles the piece
        monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
        for name in ("fq", "fa_w60", "fq_w7", "fq_crlf", "fa_crlf_w60", "fa_cr_alone_last_byte", "fq_cr_last_byte", "junk_in_front", "fq_at_plus_w5", "empty_lines"):
            for ov, cs in ((49, 1 << 30), (41, 3000), (49, 700)):   # (700, 3000: chunks end inside a piece's vouched records)
                got, st = same(lib, str(tmp_path / name), str_overhead=ov, chunk_size=cs)
            assert st["pieces"] >= 2 or len(files[name]) < int(piece)
        same(lib, str(tmp_path / "fq_w60.gz"), chunk_size=5000)
    monkeypatch.delenv("LQREADER_PIECE_BYTES")


def check_with_device_inflate(lib, tmp_path):
    data = TF.seeded_files()["fq_w60"] * 3
    bg, gz = str(tmp_path / "w60.bgz.fq.gz"), str(tmp_path / "w60.fq.gz")
    open(bg, "wb").write(bam_writer.bgzf(data, block_payload=9000))
    with gzip.open(gz, "wb", compresslevel=6) as f:
        f.write(data)
    n = len(TF.kseq_records(data)[0])
    for path in (bg, gz):
        want, _ = chunks(lib, path, chunk_size=20000, parse="host", inflate="host")
        got, fc = chunks(lib, path, chunk_size=20000, parse="device", inflate="device")
        assert got == want and got[-1][1] == n and fc.parse_stats["records_device"] > n // 2


def check_run_file(lib, tmp_path):
    from longqc_amd import synth
    T, _ = synth.make_dataset(synth.CONFIGS["tiny"])
    path = str(tmp_path / "tiny.fq")
    synth.write_fastq(path, T)
    kw = dict(adp5=TF.ADP5, adp3=TF.ADP3, nsample=20, inds=100000, gc_draw="device", gc_seed=3, suffix="x", lib=lib)
    out = []
    for tag, parse in (("h", None), ("d", "device")):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "ont-ligation", **kw)
        np.random.seed(11)
        res = p.run_file(path, chunk_size=150000, str_overhead=49, parse=parse) if parse else p.run_file(path, chunk_size=150000, str_overhead=49)
        p.mask.close_pool()
        out.append((res, open(p.mask.get_outfile_path(), "rb").read(), p.s_reads, p.gc.json_block(), p.gc.r_frac.tobytes(), p.gc.c_frac.tobytes(),
                    p.adapters.json_block(), (p.cum_n_seq, p.chunk_n, p.n_bases)))
        p.close()
    assert out[0] == out[1] and len(out[0][0]) >= 3 and out[0][1].count(b"\n") == len(T)


def error_text(lib, path, parse, **kw):
    with pytest.raises(api.LqcovError) as e:
        list(chunkpass.FileChunks(path, lib=lib, parse=parse, **kw))
    return e.value.code, str(e.value)


def check_errors(lib, tmp_path):
    L = chunkpass._lib(lib)
    missing = str(tmp_path / "no_such_file.fq")
    assert error_text(lib, missing, "device") == error_text(lib, missing, "host")
    bad = str(tmp_path / "name.fq")
    open(bad, "wb").write(b"@ok\nACGT\n+\nIIII\n@caf\xc3\xa9\nACGT\n+\nIIII\n")
    code, text = error_text(lib, bad, "device")
    assert (code, text) == error_text(lib, bad, "host") and code == -5 and "0x80" in text and "read 2" in text
    cut = str(tmp_path / "cut.fq")
    open(cut, "wb").write(b"@a\nACGT\n+\nIIII\n@b\nAC\nGT\n+\nII\nII\n@c\nACGTACGT\n+\nIIII\n")
    for cs in (1 << 30, 1):
        got, st = same(lib, cut, chunk_size=cs)
        assert [r for c in got for r in c[5]] == [["a", "ACGT", "IIII"], ["b", "ACGT", "IIII"]] and st["records_device"] == 2
    # the mode is final with the first chunk
    r = L.lqreader_open(cut.encode(), 0, 1 << 30, 1, 49, 0)
    ch = chunkpass.ReadChunk(None, lib=lib)
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert L.lqreader_parse(r, 7) == -1 and L.lqreader_parse(r, 1) == 0 and L.lqreader_parse(r, 0) == 0 and L.lqreader_parse(r, 1) == 0
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == 2
    assert L.lqreader_parse(r, 0) == -4 and b"lqreader_parse" in L.lqreader_last_error(r)
    L.lqreader_close(r)
    ch.close()
    with pytest.raises(ValueError):
        chunkpass.FileChunks(cut, lib=lib, parse="gpu")


def check_bam(lib, tmp_path):
    reads = [(b"b%d" % i, bytes(np.random.default_rng(i).choice(np.frombuffer(b"ACGT", np.uint8), 50 + 7 * i))) for i in range(40)]
    path = str(tmp_path / "x.bam")
    bam_writer.write_bam(path, reads, block_payload=700)
    want, _ = chunks(lib, path, chunk_size=3000)
    got, fc = chunks(lib, path, chunk_size=3000, parse="device")
    assert got == want and got[-1][1] == 40 and fc.format == 1 and fc.parse_stats["scans"] == 0


def check_stats(lib, tmp_path, monkeypatch):
    """a host-only path would pass every comparison above: on clean files the device must have found the records"""
    rng = np.random.default_rng(8)
    recs = [[b"read%d" % i, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(100, 300)))), b""] for i in range(2000)]
    for r in recs:
        r[2] = bytes(rng.integers(33, 127, len(r[1])).astype(np.uint8))
    fq, fa = str(tmp_path / "clean.fq"), str(tmp_path / "clean.fa")
    open(fq, "wb").write(TF.fastq_bytes(recs))
    open(fa, "wb").write(TF.fasta_bytes(recs, 60))
    monkeypatch.setenv("LQREADER_PIECE_BYTES", "65536")             # a record has at most 620 bytes: 100 records and more per piece
    for path in (fq, fa):
        got, st = same(lib, path, chunk_size=300000)
        print(path, st)
        assert len(got) >= 3 and got[-1][1] == 2000
        assert st["pieces"] >= 4 and st["records_host"] <= st["pieces"] + 1
        assert st["fallbacks"] == 0
        assert st["records_device"] + st["records_host"] == 2000


CHECKS = [check_parity, check_with_device_inflate, check_run_file, check_errors, check_bam, check_stats]


def run(check, lib, tmp_path, monkeypatch):
    names = check.__code__.co_varnames[:check.__code__.co_argcount]
    check(*[dict(lib=lib, tmp_path=tmp_path, monkeypatch=monkeypatch)[k] for k in names])


@pytest.mark.parametrize("order", LC.ORDERS)
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_emulated_device_parse(emu_lib, tmp_path, monkeypatch, check, order):
    LC.set_order(monkeypatch, order)
    run(check, emu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_gpu_device_parse(gpu_lib, tmp_path, monkeypatch, check):
    run(check, gpu_lib, tmp_path, monkeypatch)

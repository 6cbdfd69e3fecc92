"""Unaligned BAM through the chunk loop's source (chunkpass.FileChunks over lqreader_*: reader.cpp, bgzf.hpp, kernels_bam.hpp), under
the wave emulator and on the GPU -- what lq_utils.open_seq_chunk / parse_bam_chunk (lq_utils.py:238-261) yield for file_code 0:
  1. the records of a BAM chunk are the reads written, with '!' qualities; the flat bytes are those of the FASTQ path over the same
     reads; the chunks end where parse_bam_chunk ends them -- for every block size, stored and deflated blocks, empty blocks, a file
     without the EOF marker, pieces shorter than a record and 1, 3 and 16 inflate threads;
  2. is_sequel=False: chr(q + 33), '!' for a record without qualities;
  3. SampleQCPass.run_file(bam) leaves what run_file(fastq of the same reads) leaves;
  4. errors name their cause and end the reader;
  5. a bgzip-style FASTQ is still a FASTQ.
The files are written by tests/bam_writer.py from the SAM/BAM specification: the expected records are the list the test wrote."""
import ctypes as C
import itertools
import random
import struct

import numpy as np
import pytest

from longqc_amd import api, chunkpass, sampleqc, synth
from tests import bam_writer as BW
from tests import test_filechunks as TF
from tests import test_launch_caps as LC

LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 3001, 5123, 7777)
HEADER_TEXT = b"@HD\tVN:1.5\tSO:unknown\n"


def seeded_reads(seed=2):
    """-> reads [name, seq] (bytes), cigars, tags, flags: the lengths of LENS shuffled and a run of 40 reads of 0..3 bases; all 16
    codes; names of 1..40 bytes (some with a blank), 0..3 cigar operations and 0..50 tag bytes in front of / behind the sequences"""
    rng = random.Random(seed)
    lens = list(LENS)
    rng.shuffle(lens)
    lens = lens[:8] + [rng.randint(0, 3) for _ in range(40)] + lens[8:] + [5, 0, 0]
    reads, cigars, tags, flags = [], [], [], []
    for i, l in enumerate(lens):
        stem = b"m%d/%d" % (i, l)
        name = (stem + (b" ccs" if i % 7 == 3 else b"") + b"x" * 40)[:max(1, i % 40 + 1)] if i else b"q"
        reads.append([name, bytes(rng.choice(BW.CODES) for _ in range(l))])
        cigars.append([rng.randrange(1 << 32) for _ in range(rng.randint(0, 3))])
        tags.append(bytes(rng.randrange(256) for _ in range(rng.randint(0, 50))))
        flags.append(rng.choice((4, 0, 16, 256, 2048, 77)))
    return reads, cigars, tags, flags


def as_reads(reads, quals=None):
    return [[n.decode("ascii"), s.decode("ascii"), "!" * len(s) if quals is None else quals[i]] for i, (n, s) in enumerate(reads)]


def flat(L, ch):
    total = int(ch.lens.sum())
    seq, qual = np.zeros(max(total, 1), np.uint8), np.zeros(max(total, 1), np.uint8)
    assert L.lqchunk_get_reads(ch.h, 0, None, seq.ctypes.data, qual.ctypes.data) == 0
    return seq[:total].tobytes(), qual[:total].tobytes()


# ---- 1. records ----
def check_records(lib, tmp_path, monkeypatch):
    L = chunkpass._lib(lib)
    reads, cigars, tags, flags = seeded_reads()
    want = as_reads(reads)
    n, total = len(reads), sum(len(r[1]) for r in reads)
    assert set(b"".join(r[1] for r in reads)) == set(BW.CODES) and {len(r[0]) for r in reads} >= set(range(1, 41))
    # where the packed sequences start: every residue mod 16 in the inflated stream, and behind the header (which need not go up)
    hdr = len(BW.header(HEADER_TEXT))
    at, src, dst, d = hdr, [], [], 0
    for r, cg, tg in zip(reads, cigars, tags):
        rec = BW.record(r[0], r[1], None, cg, tg)
        src.append(at + 36 + len(r[0]) + 1 + 4 * len(cg))
        dst.append(d)
        at += len(rec); d += len(r[1])
    with_bases = [i for i in range(n) if len(reads[i][1])]
    assert {src[i] % 16 for i in with_bases} == set(range(16)) == {(src[i] - hdr) % 16 for i in with_bases}
    assert {dst[i] % 16 for i in with_bases} == set(range(16))
    assert any(all(len(reads[j][1]) <= 3 for j in range(i, i + 20)) for i in range(n - 20))      # one destination word spans many reads
    # the existing path over the same reads as a one-line FASTQ ('=' has no letter there: '=')
    fq = str(tmp_path / "same.fq")
    open(fq, "wb").write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r[1], b"!" * len(r[1])) for i, r in enumerate(reads)))
    ref = [flat(L, ch) for ch, _, _ in chunkpass.FileChunks(fq, chunk_size=1 << 40, is_upper=False, lib=lib)]
    assert len(ref) == 1 and ref[0][0] == b"".join(r[1] for r in reads) and ref[0][1] == b"!" * total

    def one(path, threads, what):
        got = []
        fc = chunkpass.FileChunks(path, chunk_size=1 << 40, lib=lib, n_threads=threads)
        for ch, n_seqs, n_bases in fc:
            assert fc.format == 1
            got.append((ch.records(), n_seqs, n_bases, ch.names, ch.lens.tolist(), flat(L, ch)))
        assert len(got) == 1, what
        recs, n_seqs, n_bases, names, lens, fl = got[0]
        assert (n_seqs, n_bases) == (n, total) and names == [r[0] for r in want] and lens == [len(r[1]) for r in want], what
        if recs != want:
            bad = [i for i, (g, w) in enumerate(zip(recs, want)) if g != w]
            raise AssertionError("%s: %d records against %d, first difference at %s: %r != %r" % (
                what, len(recs), len(want), bad[:1], recs[bad[0]] if bad else None, want[bad[0]] if bad else None))
        assert fl == ref[0], what

    cases = [(bp, lv, 0, True) for bp in (37, 4096, 65280) for lv in (0, 6)] + [(4096, 6, 5, True), (37, 6, 0, False)]
    for bp, lv, every, eof in cases:
        path = str(tmp_path / ("r_%d_%d_%d_%d.bam" % (bp, lv, every, eof)))
        stream = BW.write_bam(path, reads, None, bp, lv, HEADER_TEXT, (), cigars, tags, flags, eof, every)
        assert stream[:4] == b"BAM\1" and len(stream) > 4096 * 4
        for piece, threads in itertools.product((None, "4096"), (1, 3, 16)):
            if piece:
                monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
            else:
                monkeypatch.delenv("LQREADER_PIECE_BYTES", raising=False)
            one(path, threads, "block_payload %d, level %d, empty_block_every %d, eof %s, piece %s, %d threads" % (bp, lv, every, eof, piece, threads))
    monkeypatch.delenv("LQREADER_PIECE_BYTES", raising=False)
    # a header with references that spans many blocks and is longer than a piece
    path = str(tmp_path / "refs.bam")
    BW.write_bam(path, reads, None, 37, 6, b"@CO\t" + b"x" * 9000 + b"\n", [(b"chr%d" % i, 1000 + i) for i in range(30)], cigars, tags, flags)
    monkeypatch.setenv("LQREADER_PIECE_BYTES", "4096")
    one(path, 3, "a long header with references")
    monkeypatch.delenv("LQREADER_PIECE_BYTES")
    # the chunk rule: parse_bam_chunk's borders, cumulative counts, one more chunk after the last record
    path = str(tmp_path / "r_4096_6_0_1.bam")
    size = lambda ov: sum(3 * ov + len(r[0]) + 2 * len(r[1]) for r in want)
    for ov in (49, 41):
        for cs in (size(ov) // 4 + 1, 2000):
            ref_c = TF.ref_chunks(want, cs, ov)
            got = [(ch.records(), ns, nb) for ch, ns, nb in chunkpass.FileChunks(path, chunk_size=cs, str_overhead=ov, lib=lib)]
            assert [(len(c), ns, nb) for c, ns, nb in got] == [(len(c), ns, nb) for c, ns, nb in ref_c] and len(got) >= 4, (ov, cs)
            assert [c for c, _, _ in got] == [c for c, _, _ in ref_c]
    a = [x[1] for x in TF.ref_chunks(want, size(49) // 4 + 1, 49)]
    assert a != [x[1] for x in TF.ref_chunks(want, size(49) // 4 + 1, 41)]      # (the two overheads cut at different reads)
    empty = str(tmp_path / "empty.bam")
    BW.write_bam(empty, [])
    assert [(ch.records(), ns, nb) for ch, ns, nb in chunkpass.FileChunks(empty, lib=lib)] == [([], 0, 0)]


# ---- 2. is_sequel=False ----
def check_qualities(lib, tmp_path):
    L = chunkpass._lib(lib)
    rng = random.Random(8)
    reads, cigars, tags, _ = seeded_reads(4)
    quals = [bytes(rng.randint(0, 93) for _ in r[1]) for r in reads]
    quals[0] = bytes(range(94)); reads[0][1] = bytes(rng.choice(b"ACGT") for _ in range(94))      # every value once
    none = [i for i, r in enumerate(reads) if i % 9 == 4 and len(r[1])]
    assert len(none) >= 3 and any(len(reads[i][1]) > 16 for i in none)
    for i in none:
        quals[i] = None
    path = str(tmp_path / "q.bam")
    BW.write_bam(path, reads, quals, 4096, 6, HEADER_TEXT, (), cigars, tags)
    want = as_reads(reads, ["!" * len(r[1]) if q is None else bytes(x + 33 for x in q).decode("latin-1") for r, q in zip(reads, quals)])
    assert want[0][2] == bytes(range(33, 127)).decode()
    got = [ch.records() for ch, _, _ in chunkpass.FileChunks(path, lib=lib, is_sequel=False)]
    assert got == [want]
    got = [ch.records() for ch, _, _ in chunkpass.FileChunks(path, lib=lib)]                          # the default: '!' throughout
    assert got == [as_reads(reads)]
    # valid before the first lqreader_next only
    r = L.lqreader_open(path.encode(), 0, 1 << 30, 1, 49, 0)
    assert r and L.lqreader_format(r) == 1 and L.lqreader_bam_qualities(r, 1) == 0 and L.lqreader_bam_qualities(r, 0) == 0
    ch = chunkpass.ReadChunk(None, lib=lib)
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert L.lqreader_next(r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last)) == 0 and n.value == len(reads) and last.value == 1
    assert L.lqreader_bam_qualities(r, 1) == -4 and b"lqreader_bam_qualities" in L.lqreader_last_error(r)
    L.lqreader_close(r)
    ch.close()


# ---- 3. the whole loop ----
def check_whole_loop(lib, tmp_path, with_coverage):
    cfg = synth.SynthConfig("bam", n_reads=300, mean_len=2500, depth=8.0, seed=7103, nsample=40)
    T, _ = synth.make_dataset(cfg)
    short = 0
    for i in range(0, len(T), 11):                                  # some reads shorter than a GC window
        T.seqs[i], T.quals[i] = T.seqs[i][:20 + i % 120], T.quals[i][:20 + i % 120]
        short += 1
    assert len(T) == 300 and short > 20 and sum(1 for s in T.seqs if s.shape[0] < 150) >= short
    fq, bam = str(tmp_path / "w.fq"), str(tmp_path / "w.bam")
    for i in range(len(T)):
        T.quals[i] = np.full(T.seqs[i].shape[0], 33, np.uint8)      # what parse_bam_chunk gives every read
    synth.write_fastq(fq, T)
    BW.write_bam(bam, [(nm.encode(), s.tobytes()) for nm, s in zip(T.names, T.seqs)], None, 65280, 6)
    adp5, adp3 = sampleqc.PRESET_ADAPTERS["pb-sequel"]
    cs = sum(3 * 49 + len(nm) + 2 * s.shape[0] for nm, s in zip(T.names, T.seqs)) // 4 + 1
    out = []
    for tag, path in (("a", bam), ("b", fq)):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "pb-sequel", adp5=adp5, adp3=adp3, nsample=40, inds=200000, gc_draw="device",
                                   gc_seed=3, suffix="x", lib=lib)
        np.random.seed(11)
        res = p.run_file(path, chunk_size=cs, str_overhead=49)
        p.mask.close_pool()
        out.append((p, res))
    (a, ra), (b, rb) = out
    assert len(ra) >= 4 and ra == rb
    table = open(a.mask.get_outfile_path(), "rb").read()
    assert table == open(b.mask.get_outfile_path(), "rb").read() and table.count(b"\n") == 300
    assert a.s_reads == b.s_reads and len(a.s_reads) == 40 and all(a.s_reads)
    assert a.gc.r_frac.tobytes() == b.gc.r_frac.tobytes() and a.gc.c_frac.tobytes() == b.gc.c_frac.tobytes() and len(a.gc.c_frac) > 0
    assert a.adapters.json_block() == b.adapters.json_block() and a.gc.json_block() == b.gc.json_block()
    assert (a.cum_n_seq, a.chunk_n, a.n_bases) == (b.cum_n_seq, b.chunk_n, b.n_bases) == (300, len(ra), T.n_bases)
    if with_coverage:
        text = a.coverage()
        assert text == b.coverage() and sum(1 for l in text.splitlines() if l.split("\t")[2] != "0") > 10
    a.close(); b.close()


# ---- 4. errors ----
def check_errors(lib, tmp_path):
    L = chunkpass._lib(lib)
    reads = [[b"r%d" % i, b"ACGTNACGTN" * (3 + i)] for i in range(40)]
    stream = BW.bam_stream(reads)
    whole = BW.bgzf(stream, 300)
    blocks, at = [], 0                                              # where the blocks begin
    while at < len(whole):
        blocks.append(at)
        at += struct.unpack_from("<H", whole, at + 16)[0] + 1
    assert len(blocks) > 8 and at == len(whole)
    rec1 = len(BW.header()) + len(BW.record(*reads[0]))              # the second record's block_size
    assert struct.unpack_from("<i", stream, rec1)[0] == len(BW.record(*reads[1])) - 4

    def damaged(**kw):
        s = bytearray(stream)
        if "block_size" in kw:
            s[rec1:rec1 + 4] = struct.pack("<i", kw["block_size"])
        if "name" in kw:
            s[rec1 + 36:rec1 + 36 + len(kw["name"])] = kw["name"]
        return BW.bgzf(bytes(s), 300)

    flipped = bytearray(whole)
    flipped[blocks[3] + 18 + 5] ^= 0x40                              # inside the fourth block's deflate bytes
    cases = [("cut_in_block", whole[:blocks[5] + 40], -2, ("cut short",)),
             ("cut_between_blocks", whole[:blocks[5]], -2, ("ends inside a record",)),
             ("crc", bytes(flipped), -2, ("CRC32", "deflate", "ISIZE")),
             ("block_size", damaged(block_size=40), -2, ("block_size", "too small")),
             ("no_nul", damaged(name=b"r1x"), -2, ("NUL",)),
             ("high_byte", damaged(name=b"\xc3\xa9"), -5, ("0x80",))]
    ends = set(np.cumsum([len(BW.header())] + [len(BW.record(*r)) for r in reads]).tolist())
    assert 300 * 5 not in ends and 300 * 5 > min(ends)              # (the cut between blocks falls into a record, not between two)
    ch = chunkpass.ReadChunk(None, lib=lib)
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    for name, data, code, words in cases:
        path = str(tmp_path / (name + ".bam"))
        open(path, "wb").write(data)
        with pytest.raises(api.LqcovError) as e:
            list(chunkpass.FileChunks(path, lib=lib))
        assert e.value.code == code and any(w in str(e.value) for w in words), (name, str(e.value))
        if name == "crc":
            assert str(blocks[3]) in str(e.value)                   # the block is named by its place in the file
        for cs in (1 << 30, 1):                                     # the reader then refuses next
            r = L.lqreader_open(path.encode(), 0, cs, 1, 49, 0)
            assert r and L.lqreader_format(r) == 1
            args = (r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last))
            rc = L.lqreader_next(*args)
            while rc == 0 and not last.value:
                rc = L.lqreader_next(*args)
            assert rc == code and any(w.encode() in L.lqreader_last_error(r) for w in words), (name, cs)
            assert L.lqreader_next(*args) == -4
            L.lqreader_close(r)
    ch.close()
    # the whole file is fine
    path = str(tmp_path / "whole.bam")
    open(path, "wb").write(whole)
    assert [c.records() for c, _, _ in chunkpass.FileChunks(path, lib=lib)] == [as_reads(reads)]


# ---- 5. detection ----
def check_detection(lib, tmp_path):
    recs = TF.rand_records(11)
    data = TF.fastq_bytes(recs)
    path = str(tmp_path / "bgzip.fq.gz")
    open(path, "wb").write(BW.bgzf(data, 4096))
    fc = chunkpass.FileChunks(path, lib=lib)
    got = [ch.records() for ch, _, _ in fc]
    assert fc.format == 0 and got == [TF.as_reads(TF.kseq_records(data)[0])] and len(got[0]) == len(recs)
    bam = str(tmp_path / "d.bam")
    BW.write_bam(bam, [(b"a", b"ACGT")])
    fc = chunkpass.FileChunks(bam, lib=lib)
    assert fc.format is None and [ch.records() for ch, _, _ in fc] == [[["a", "ACGT", "!!!!"]]] and fc.format == 1


# ---- the emulator build ----
@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_bam_records(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_records(emu_lib, tmp_path, monkeypatch)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_bam_qualities_from_the_file(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_qualities(emu_lib, tmp_path)


def test_emulated_run_file_on_a_bam_equals_run_file_on_its_fastq(emu_lib, tmp_path):
    check_whole_loop(emu_lib, tmp_path, with_coverage=False)


def test_emulated_bam_errors(emu_lib, tmp_path):
    check_errors(emu_lib, tmp_path)


def test_emulated_bam_detection(emu_lib, tmp_path):
    check_detection(emu_lib, tmp_path)


# ---- the gfx950 build ----
@pytest.mark.gpu
def test_gpu_bam_records(gpu_lib, tmp_path, monkeypatch):
    check_records(gpu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_bam_qualities_from_the_file(gpu_lib, tmp_path):
    check_qualities(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_run_file_on_a_bam_equals_run_file_on_its_fastq(gpu_lib, tmp_path):
    check_whole_loop(gpu_lib, tmp_path, with_coverage=True)


@pytest.mark.gpu
def test_gpu_bam_errors(gpu_lib, tmp_path):
    check_errors(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_bam_detection(gpu_lib, tmp_path):
    check_detection(gpu_lib, tmp_path)

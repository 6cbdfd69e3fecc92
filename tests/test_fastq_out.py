"""Trimmed reads and converted FASTQ written from the resident chunk (k_fastq_format, lqchunk_fastq, lqfastq_*, chunkpass.FastqWriter,
SampleQCPass.run_file(trim=<path>, fastx_out=<path>)) against the project's own host path: adapter.cut_adapter on chunk.records(),
written by sampleqc.write_fastq(fn, records, is_chunk=True).
  1. adapter.trim_bounds holds exactly what adapter._cut leaves of the records (no library);
  2. the text of a chunk, byte for byte, trimmed and untrimmed, in one launch and in pieces of one tile;
  3. run_file(trim=<path>) writes the file of run_file(trim=True) + write_fastq and changes nothing else, without fetching the reads;
  4. run_file(fastx_out=<path>) on a BAM file writes the FASTQ of its records;
  5. refused arguments and failing files."""
import os

import numpy as np
import pytest

from longqc_amd import adapter, api, chunkpass, sampleqc
from tests import bam_writer
from tests import test_launch_caps as LC
from tests.conftest import GOLDEN

ADP5, ADP3 = sampleqc.PRESET_ADAPTERS["ont-ligation"]
TILE = 4096


def text_of(records):
    return "".join("@%s\n%s\n+\n%s\n" % tuple(r) for r in records).encode("latin-1")


# ---- 1. trim_bounds ----
def rand_rows(rng, lens, length, adp_len):
    """rows a search of `length`-base windows can return for reads of these lengths: -1 for reads shorter than 2 * length, else
    0 <= s <= e < length, L around the adapter's length and d with identities 1 - d / L below, above and exactly 0.75"""
    n = lens.shape[0]
    rows = np.full((n, 4), -1, dtype=np.int32)
    for i in np.flatnonzero(lens >= 2 * length).tolist():
        L = int(rng.integers(max(1, adp_len - 8), adp_len + 9))
        kind = int(rng.integers(0, 4))
        if kind == 0:                                               # exactly 0.75: not a hit
            L = 4 * int(rng.integers(1, (adp_len + 8) // 4 + 1))
            d = L // 4
        elif kind == 1:                                             # just above
            d = max(0, (L - 1) // 4 if L % 4 else L // 4 - 1)
        else:
            d = int(rng.integers(0, L + 1))
        e = int(rng.integers(min(L, length) - 1, length))
        s = max(0, e - L + 1 + int(rng.integers(0, 3)))
        rows[i] = (d, min(s, e), e, L)
    return rows


def rand_records(rng, lens):
    out = []
    for i, l in enumerate(lens.tolist()):
        s = "".join("ACGT"[x] for x in rng.integers(0, 4, l))
        q = "".join(chr(x) for x in rng.integers(33, 127, l))
        out.append(["n%d" % i, s, q])
    return out


@pytest.mark.parametrize("which", ["5", "3", "both"])
@pytest.mark.parametrize("length", [150, 60])
def test_trim_bounds_hold_what_cut_leaves(monkeypatch, which, length):
    rng = np.random.default_rng(41 + length)
    # lengths: shorter than two windows, exactly two, such that a 5' cut (at most `length` bases) leaves fewer than two, and longer
    lens = np.concatenate([rng.integers(0, 2 * length, 60), [2 * length] * 20, rng.integers(2 * length, 3 * length + 1, 200),
                           rng.integers(3 * length, 4000, 60)]).astype(np.int64)
    rng.shuffle(lens)
    o5 = rand_rows(rng, lens, length, len(ADP5)) if which != "3" else None
    o3 = rand_rows(rng, lens, length, len(ADP3)) if which != "5" else None
    for o in (o5, o3):                                              # the rows fall on both sides of the threshold, and on it
        if o is not None:
            ident = adapter._identity(o[lens >= 2 * length])
            assert (ident == 0.75).sum() >= 10 and (ident > 0.75).sum() >= 30 and (ident < 0.75).sum() >= 30
    records = rand_records(rng, lens)
    whole = [list(r) for r in records]
    monkeypatch.setattr(adapter, "_hits", lambda seqs, a5, a3, ln, device=0, lib=None: (o5 if a5 else None, o3 if a3 else None))
    bounds = []
    res = adapter.cut_adapter(records, adp_t=ADP5 if o5 is not None else None, adp_b=ADP3 if o3 is not None else None, length=length,
                              bounds_out=bounds)                    # (_cut trims the records in place)
    begin, end = adapter.trim_bounds(o5, o3, lens, length=length)
    assert begin.dtype == end.dtype == np.uint32 and (bounds[0] == begin).all() and (bounds[1] == end).all()
    for r, w, b, e in zip(records, whole, begin.tolist(), end.tolist()):
        assert r[1] == w[1][b:e] and r[2] == w[2][b:e] and 0 <= b <= e <= len(w[1])
    n5, n3 = int((begin > 0).sum()), int((end < lens).sum())
    tuples = res if which == "both" else (res, None) if which == "5" else (None, res)
    assert (tuples[0][1] if tuples[0] else 0) == n5 and (tuples[1][1] if tuples[1] else 0) == n3
    assert (n5 >= 30 or o5 is None) and (n3 >= 30 or o3 is None)
    if which == "both":                                             # reads whose 5' cut takes them below two windows: the 3' hit does not count
        dropped = (lens >= 2 * length) & (lens - begin < 2 * length) & (adapter._identity(o3) > 0.75)
        assert dropped.sum() >= 5 and (end[dropped] == lens[dropped]).all()
    assert adapter.cut_adapter([list(r) for r in whole], adp_t=ADP5 if o5 is not None else None, adp_b=ADP3 if o3 is not None else None,
                               length=length) == res                # (without the keyword: as before)


def test_trim_bounds_without_rows_or_reads():
    b, e = adapter.trim_bounds(None, None, [5, 0, 700])
    assert b.tolist() == [0, 0, 0] and e.tolist() == [5, 0, 700]
    b, e = adapter.trim_bounds(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), np.zeros(0, np.int64))
    assert b.shape == e.shape == (0,)


# ---- 2. the text ----
def put(rng, adp, n_err):
    a = list(adp)
    for p in rng.choice(len(a), n_err, replace=False).tolist():
        a[p] = "ACGT"[("ACGT".index(a[p]) + 1) % 4]
    return "".join(a)


def seeded_records(seed):
    """names of 0..40 bytes, reads of 0, 1, 15, 16, 17, 299, 300, 301 and a few thousand bases, the preset's adapters at the 5' end, the 3'
    end, both and neither"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 15, 16, 17, 299, 300, 301, 0, 0, 2500, 4100, 3333] + rng.integers(0, 40, 30).tolist() + rng.integers(300, 1500, 40).tolist()
    out = []
    for i, l in enumerate(lens):
        s = "".join("ACGTN"[x] for x in rng.integers(0, 5, l))
        if l >= 300 and i % 4 != 3:
            k = i % 4                                               # 0: 5' only, 1: 3' only, 2: both
            if k in (0, 2):
                s = s[:3] + put(rng, ADP5, 2) + s[3 + len(ADP5):]
            if k in (1, 2):
                s = s[:l - 5 - len(ADP3)] + put(rng, ADP3, 1) + s[l - 5:]
            assert len(s) == l
        name = "" if i in (8, 20) else "".join(chr(x) for x in rng.integers(48, 123, int(rng.integers(1, 41))))
        out.append([name, s, "".join(chr(x) for x in rng.integers(33, 127, l))])
    assert {len(r[0]) for r in out} >= {0, 1, 40} or len({len(r[0]) for r in out}) > 20
    return out


def check_chunk_text(lib, tmp_path, chunk, tag, want_all_kinds=False):
    """every way to the chunk's text against the host path, trimmed by both adapters, by one, and untrimmed"""
    whole = chunk.records()
    lens = np.array([len(r[1]) for r in whole], dtype=np.int64)
    for k, (a5, a3) in enumerate(((ADP5, ADP3), (ADP5, None), (None, ADP3), (None, None))):
        records = [list(r) for r in whole]
        bounds = []
        if a5 or a3:
            want_tuples = adapter.cut_adapter(records, adp_t=a5, adp_b=a3, chunk=chunk, lib=lib)
            assert adapter.cut_adapter(None, adp_t=a5, adp_b=a3, chunk=chunk, lib=lib, bounds_out=bounds) == want_tuples
            begin, end = bounds
            if want_all_kinds and a5 and a3:                        # reads with a 5' hit only, a 3' hit only, both and none
                h5, h3 = begin > 0, end < lens
                assert (h5 & ~h3).sum() >= 3 and (~h5 & h3).sum() >= 3 and (h5 & h3).sum() >= 3 and (~h5 & ~h3 & (lens >= 300)).sum() >= 3
        else:
            bounds = [None, None]
        want = text_of(records)
        assert chunk.fastq_bytes(*bounds) == want
        for piece in (TILE, None):
            fn = str(tmp_path / ("%s_%d_%s.fq" % (tag, k, piece)))
            with chunkpass.FastqWriter(fn, piece_bytes=piece, lib=lib) as w:
                assert w.write(chunk, *bounds) == len(want)
                assert w.write(chunk, *bounds) == len(want)         # (a second write appends)
            assert open(fn, "rb").read() == want + want
            assert len(want) > 3 * TILE or not want_all_kinds       # pieces of one tile: borders inside records


def check_text(lib, tmp_path):
    # a seeded chunk from lists and from a file
    recs = seeded_records(5)
    ch = chunkpass.ReadChunk(recs, lib=lib)
    assert ch.records() == recs
    check_chunk_text(lib, tmp_path, ch, "lists", want_all_kinds=True)
    ch.load([])                                                     # an empty chunk: no text, no file
    assert ch.fastq_bytes() == b""
    fn = str(tmp_path / "empty.fq")
    with chunkpass.FastqWriter(fn, lib=lib) as w:
        assert w.write(ch) == 0
    assert not os.path.exists(fn)
    ch.close()
    path = str(tmp_path / "seeded.fq")
    named = [r for r in recs if r[0]]                               # (a record without a name is not a FASTQ record)
    open(path, "wb").write(text_of(named))
    n_chunks = 0
    for ch, _, _ in chunkpass.FileChunks(path, chunk_size=40000, is_upper=False, lib=lib):
        check_chunk_text(lib, tmp_path, ch, "file%d" % n_chunks)
        n_chunks += 1
    assert n_chunks >= 3
    # the golden files, through the reader and from lists
    for fn in ("tiny_sub.fq.gz", "tiny_all.fq.gz", "adv_sub.fq.gz"):
        n_reads = 0
        for ch, _, _ in chunkpass.FileChunks(os.path.join(GOLDEN, fn), chunk_size=100000, is_upper=False, lib=lib):
            recs = ch.records()
            assert ch.fastq_bytes() == text_of(recs)
            n_reads += ch.n
            if fn == "tiny_sub.fq.gz" and ch.n:
                check_chunk_text(lib, tmp_path, ch, "golden%d" % n_reads)
                listed = chunkpass.ReadChunk(recs, lib=lib)
                check_chunk_text(lib, tmp_path, listed, "golden_lists%d" % n_reads)
                listed.close()
        assert n_reads > 10


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_text_equals_the_host_path(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_text(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_text_equals_the_host_path(gpu_lib, tmp_path):
    check_text(gpu_lib, tmp_path)


# ---- 3. run_file(trim=<path>) ----
def adapter_file(tmp_path):
    rng = np.random.default_rng(77)
    recs = []
    for i in range(120):
        l = int(rng.integers(300, 2500)) if i % 5 else int(rng.integers(0, 300))
        s = "".join("ACGT"[x] for x in rng.integers(0, 4, l))
        if l >= 300 and i % 3 == 0:
            s = s[:4] + put(rng, ADP5, 1) + s[4 + len(ADP5):]
        if l >= 300 and i % 4 == 0:
            s = s[:l - 2 - len(ADP3)] + put(rng, ADP3, 1) + s[l - 2:]
        recs.append(["read%d" % i, s, "".join(chr(x) for x in rng.integers(33, 127, l))])
    path = str(tmp_path / "adapters.fq")
    open(path, "wb").write(text_of(recs))
    return path, recs


def check_run_file_trim(lib, tmp_path, monkeypatch):
    path, recs = adapter_file(tmp_path)
    cs, nsample = 60000, 15
    kw = dict(adp5=ADP5, adp3=ADP3, nsample=nsample, gc_draw="device", gc_seed=3, suffix="x", lib=lib)
    # the parent path: every record to the host, trimmed there, written chunk by chunk
    b = chunkpass.SampleQCPass(str(tmp_path / "b"), "ont-ligation", **kw)
    np.random.seed(11)
    want = b.run_file(path, chunk_size=cs, trim=True, str_overhead=49)
    want_fn = str(tmp_path / "want.fq")
    for t in b.trimmed_chunks:
        sampleqc.write_fastq(want_fn, t, is_chunk=True)
    assert len(want) >= 4 and sum(t[0][1] for t in want) > 5 and sum(t[1][1] for t in want) > 5     # (>= 3 chunks and the empty last one)
    assert open(want_fn, "rb").read() != text_of(recs)
    # the new path, counting what records() fetches
    fetched = []
    real = chunkpass.ReadChunk.records

    def counting(self, idx=None):
        fetched.append(self.n if idx is None else len(idx))
        return real(self, idx)
    monkeypatch.setattr(chunkpass.ReadChunk, "records", counting)
    a = chunkpass.SampleQCPass(str(tmp_path / "a"), "ont-ligation", **kw)
    np.random.seed(11)
    got_fn = tmp_path / "got.fq"                                    # (an os.PathLike)
    got = a.run_file(path, chunk_size=cs, trim=got_fn, str_overhead=49)
    monkeypatch.setattr(chunkpass.ReadChunk, "records", real)
    assert fetched and max(fetched) <= nsample and sum(fetched) < len(recs)
    assert got == want and a.trimmed is None and a.trimmed_chunks == []
    assert open(got_fn, "rb").read() == open(want_fn, "rb").read()
    for p in (a, b):
        p.mask.close_pool()
    assert open(a.mask.get_outfile_path(), "rb").read() == open(b.mask.get_outfile_path(), "rb").read()
    assert a.adapters.json_block() == b.adapters.json_block() and len(a.adapters.json_block()) == 2
    assert a.gc.json_block() == b.gc.json_block() and a.gc.gc_stats() == b.gc.gc_stats()
    assert a.gc.r_frac.tobytes() == b.gc.r_frac.tobytes() and a.gc.c_frac.tobytes() == b.gc.c_frac.tobytes() and len(a.gc.c_frac) > 0
    assert a.s_reads == b.s_reads and len(a.s_reads) == nsample and all(a.s_reads)
    assert (a.cum_n_seq, a.chunk_n, a.n_bases) == (b.cum_n_seq, b.chunk_n, b.n_bases)
    # fastx_out beside it: the untrimmed reads, for any input
    c = chunkpass.SampleQCPass(str(tmp_path / "c"), "ont-ligation", **kw)
    np.random.seed(11)
    assert c.run_file(path, chunk_size=cs, trim=str(tmp_path / "got2.fq"), fastx_out=str(tmp_path / "all.fq"), str_overhead=49) == want
    assert open(tmp_path / "all.fq", "rb").read() == text_of(recs) and open(tmp_path / "got2.fq", "rb").read() == open(want_fn, "rb").read()
    # a loop that raises still closes the writers; a file that cannot be made is reported
    d = chunkpass.SampleQCPass(str(tmp_path / "d"), "ont-ligation", **kw)
    with monkeypatch.context() as m:
        m.setattr(chunkpass.SampleQCPass, "add_resident", lambda self, chunk, trim=False: 1 / 0)
        with pytest.raises(ZeroDivisionError):
            d.run_file(path, chunk_size=cs, trim=str(tmp_path / "got3.fq"), fastx_out=str(tmp_path / "all3.fq"), str_overhead=49)
    assert d.trim_writer.h is None and d.fastx_writer.h is None
    with pytest.raises(api.LqcovError) as e:
        d.run_file(path, chunk_size=cs, trim=str(tmp_path / "no_such_dir" / "got.fq"), str_overhead=49)
    assert e.value.code == -2 and "no_such_dir" in str(e.value) and d.trim_writer.h is None
    for p in (a, b, c, d):
        p.close()


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_run_file_writes_the_trimmed_reads(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_run_file_trim(emu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_run_file_writes_the_trimmed_reads(gpu_lib, tmp_path, monkeypatch):
    check_run_file_trim(gpu_lib, tmp_path, monkeypatch)


# ---- 4. fastx_out on a BAM file ----
def check_bam_fastx(lib, tmp_path):
    rng = np.random.default_rng(9)
    reads, quals = [], []
    for i in range(90):
        l = int(rng.integers(0, 40)) if i % 6 == 0 else int(rng.integers(300, 3000))
        reads.append((b"m64/%d/ccs" % i, bytes(b"=ACMGRSVTWYHKDBN"[x] for x in rng.integers(0, 16, l))))
        quals.append(None if i % 7 == 0 else bytes(rng.integers(0, 94, l).astype(np.uint8)))
    path = str(tmp_path / "reads.bam")
    bam_writer.write_bam(path, reads, quals, block_payload=20000)
    for is_sequel in (True, False):
        want_fn, got_fn = str(tmp_path / ("want%d.fq" % is_sequel)), str(tmp_path / ("got%d.fq" % is_sequel))
        n_chunks = 0
        for ch, _, _ in chunkpass.FileChunks(path, chunk_size=50000, str_overhead=49, is_sequel=is_sequel, lib=lib):
            sampleqc.write_fastq(want_fn, ch.records(), is_chunk=True)
            n_chunks += 1
        assert n_chunks >= 4
        p = chunkpass.SampleQCPass(str(tmp_path / ("bam%d" % is_sequel)), "ont-ligation", adp5=ADP5, adp3=ADP3, nsample=10, suffix="x", lib=lib)
        np.random.seed(11)
        res = p.run_file(path, chunk_size=50000, str_overhead=49, is_sequel=is_sequel, fastx_out=got_fn)
        assert len(res) == n_chunks and p.trimmed is None and p.trimmed_chunks == []
        want = open(want_fn, "rb").read()
        assert open(got_fn, "rb").read() == want and want.count(b"\n") == 4 * len(reads)
        assert (b"\n+\n!!!!" in want) and ((want.count(b"!") == sum(len(r[1]) for r in reads)) == is_sequel)
        p.mask.close_pool()
        p.close()


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_fastx_out_of_a_bam_file(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_bam_fastx(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_fastx_out_of_a_bam_file(gpu_lib, tmp_path):
    check_bam_fastx(gpu_lib, tmp_path)


# ---- 5. errors ----
def check_errors(lib, tmp_path):
    recs = seeded_records(6)
    ch = chunkpass.ReadChunk(recs, lib=lib)
    lens = ch.lens.astype(np.uint32)
    zeros = np.zeros(ch.n, np.uint32)
    fn = str(tmp_path / "out.fq")
    w = chunkpass.FastqWriter(fn, piece_bytes=TILE, lib=lib)
    # begin > end, end > len: refused before a byte is made; the writer stays usable
    for begin, end, what in ((np.where(lens > 2, 2, 0).astype(np.uint32), np.where(lens > 2, 1, lens).astype(np.uint32), "begin > end"),
                             (zeros, lens + (np.arange(ch.n) == 7), "end > the length")):
        for call in (lambda: w.write(ch, begin, end), lambda: ch.fastq_bytes(begin, end)):
            with pytest.raises(api.LqcovError) as e:
                call()
            assert e.value.code == -1 and what in str(e.value)
    with pytest.raises(ValueError):
        w.write(ch, zeros[:-1], lens[:-1])
    with pytest.raises(ValueError):
        ch.fastq_bytes(zeros, None)
    assert not os.path.exists(fn)
    assert w.write(ch, zeros, lens) == len(text_of(recs))
    # a chunk without qualities
    bare = chunkpass.ReadChunk([r[:2] for r in recs], lib=lib)
    for call in (lambda: w.write(bare), lambda: bare.fastq_bytes()):
        with pytest.raises(api.LqcovError) as e:
            call()
        assert e.value.code == -1 and "qualities" in str(e.value)
    w.close()
    w.close()                                                       # (closed twice: nothing)
    assert open(fn, "rb").read() == text_of(recs)
    with pytest.raises(ValueError):
        w.write(ch)
    # a path in a missing directory: every write reports it, none blocks, close returns
    w = chunkpass.FastqWriter(str(tmp_path / "missing" / "out.fq"), lib=lib)
    for _ in range(2):
        with pytest.raises(api.LqcovError) as e:
            w.write(ch)
        assert e.value.code == -2 and "failed to open" in str(e.value) and "missing" in str(e.value)
    with pytest.raises(api.LqcovError) as e:
        w.close()
    assert e.value.code == -2 and "missing" in str(e.value) and w.h is None
    # a file that takes no byte: the writer thread's error ends the write that waits for it, every later one, and close
    if os.path.exists("/dev/full"):
        w = chunkpass.FastqWriter("/dev/full", piece_bytes=TILE, lib=lib)
        assert len(text_of(recs)) > 4 * TILE                        # (more pieces than buffers: the write has to wait for the thread)
        for _ in range(2):
            with pytest.raises(api.LqcovError) as e:
                w.write(ch)
            assert e.value.code == -2 and "failed to write" in str(e.value)
        with pytest.raises(api.LqcovError) as e:
            w.close()
        assert e.value.code == -2 and "/dev/full" in str(e.value)
    with pytest.raises(api.LqcovError) as e:
        chunkpass.FastqWriter(fn, piece_bytes=TILE + 16, lib=lib)
    assert "multiple" in str(e.value)
    ch.close(); bare.close()


def test_emulated_writer_errors(emu_lib, tmp_path):
    check_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_writer_errors(gpu_lib, tmp_path):
    check_errors(gpu_lib, tmp_path)

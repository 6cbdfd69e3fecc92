"""The chunk loop's source on the device (longqc_amd/chunkpass.FileChunks over lqreader_*, reader.cpp, kernels_gather.hpp), under the
wave emulator and on the GPU:
  1. the records of a file chunk are kseq's records of the file, upper-cased and with '!' where there is no quality string -- for the
     golden files and for seeded files of every line layout, plain and gzipped, in pieces longer and shorter than a record;
  2. the low-complexity table written from file chunks is the reference binary's own for the FASTQ goldens;
  3. the chunks end where lq_utils.parse_fastx_chunk ends them, for both values of sys.getsizeof("");
  4. SampleQCPass.run_file leaves what add_chunk(reads) leaves on the same records cut at the same borders;
  5. errors: a missing file, a name that is not ASCII, a truncated last record.
kseq_records and ref_chunks below are restatements of kseq.h:93-141,184-224 (kseq_read over a stream that has ended when its last
byte is consumed: files here are no multiple of kseq's 16384-byte buffer) and of lq_utils.py:263-289 in plain Python."""
import gzip
import os
import random

import numpy as np
import pytest

from longqc_amd import adapter, api, chunkpass, gcfrac, sampleqc, sdust, synth
from tests import test_chunkpass as TC
from tests.conftest import GOLDEN, read_gz

SPACE = b" \t\n\v\f\r"


# ---- kseq, restated ----
def kseq_records(data):
    """-> (records [name, seq, qual or None] as bytes, src: the file offset of every sequence / quality line that gives bytes,
    dst: where its first byte lands in the concatenated sequences / qualities)"""
    n = len(data)
    st = {"pos": 0}
    src, dst = [], []

    def getc():
        if st["pos"] >= n:
            return -1
        st["pos"] += 1
        return data[st["pos"] - 1]

    def getuntil(space, s):
        """ks_getuntil2(..., append=1): -> (-1 at the end of the stream, else len(s)), the delimiter"""
        pos = st["pos"]
        if pos >= n:
            return -1, 0
        i = pos
        if space:
            while i < n and data[i] not in SPACE:
                i += 1
        else:
            i = data.find(b"\n", pos)
            i = n if i < 0 else i
        s += data[pos:i]
        st["pos"] = i + 1 if i < n else n
        if not space and len(s) > 1 and s[-1] == 13:
            del s[-1]
        return len(s), (data[i] if i < n else 0)

    out, last, bases = [], 0, 0
    while True:
        if last == 0:
            c = getc()
            while c != -1 and c not in (62, 64):
                c = getc()
            if c == -1:
                break
            last = c
        name = bytearray()
        r, c = getuntil(True, name)
        if r < 0:
            break
        if c != 10:
            getuntil(False, bytearray())
        seq = bytearray()
        while True:
            c = getc()
            if c == -1 or c in (62, 43, 64):
                break
            if c == 10:
                continue
            src.append(st["pos"] - 1); dst.append(bases + len(seq))
            seq.append(c)
            getuntil(False, seq)
        if c in (62, 64):
            last = c
        if c != 43:
            out.append([bytes(name), bytes(seq), None])
            bases += len(seq)
            continue
        c = getc()
        while c != -1 and c != 10:
            c = getc()
        if c == -1:
            break                                                  # -2: no quality string
        qual = bytearray()
        while True:
            at, before = st["pos"], len(qual)
            r, _ = getuntil(False, qual)
            if r > before:
                src.append(at); dst.append(bases + before)
            if not (r >= 0 and len(qual) < len(seq)):
                break
        last = 0
        if len(seq) != len(qual):
            break                                                  # -2: truncated quality, the stream ends
        out.append([bytes(name), bytes(seq), bytes(qual)])
        bases += len(seq)
    return out, src, dst


def as_reads(records, is_upper=True):
    """what lq_utils.parse_fastx_chunk makes of pysam's entries (lq_utils.py:271-281)"""
    out = []
    for name, seq, qual in records:
        s = seq.decode("latin-1")
        out.append([name.decode("ascii"), s.upper() if is_upper else s, qual.decode("latin-1") if qual else "!" * len(s)])
    return out


def ref_chunks(reads, cs, overhead):
    """lq_utils.py:263-289 with sys.getsizeof(str) = overhead + len"""
    out, cur, n_seqs, n_bases, size = [], [], 0, 0, 0
    for r in reads:
        cur.append(r)
        size += 3 * overhead + len(r[0]) + len(r[1]) + len(r[2])
        n_seqs += 1
        n_bases += len(r[1])
        if size >= cs:
            out.append((cur, n_seqs, n_bases))
            size, cur = 0, []
    out.append((cur, n_seqs, n_bases))
    return out


def file_bytes(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


# ---- seeded files ----
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 3001, 5123, 7777)


def rand_records(seed, alphabet=b"ACGTacgtuUNn", extra=40):
    rng = random.Random(seed)
    lens = list(LENS) + [rng.randint(0, 200) for _ in range(extra)]
    rng.shuffle(lens)
    out = []
    for i, l in enumerate(lens):
        name = ("r%d" % i).encode() + (b"" if i % 3 else b" a comment\twith tabs") + (b"" if i % 5 else b" x=1")
        seq = bytes(rng.choice(alphabet) for _ in range(l))
        qual = bytes(rng.randint(33, 126) for _ in range(l))
        out.append([name, seq, qual])
    return out


def wrap(s, width, eol):
    if not width:
        return s + eol
    return b"".join(s[i:i + width] + eol for i in range(0, len(s), width)) or eol


def fasta_bytes(records, width=0, eol=b"\n"):
    return b"".join(b">" + nm + eol + (wrap(s, width, eol) if s else b"") for nm, s, _ in records)


def fastq_bytes(records, width=0, eol=b"\n"):
    return b"".join(b"@" + nm + eol + wrap(s, width, eol) + b"+" + (nm if len(s) % 2 else b"") + eol + wrap(q, width, eol) for nm, s, q in records)


def seeded_files():
    """name -> bytes: every line layout of the list in the module's docstring"""
    recs = rand_records(11)
    files = {}
    for w in (1, 15, 16, 17, 60):
        files["fa_w%d" % w] = fasta_bytes(rand_records(20 + w, extra=12 if w == 1 else 40), w)
    files["fq"] = fastq_bytes(recs)
    files["fq_w60"] = fastq_bytes(recs, 60)
    files["fq_w7"] = fastq_bytes(rand_records(12, extra=10), 7)
    files["fq_crlf"] = fastq_bytes(recs, 0, b"\r\n")
    files["fa_crlf_w60"] = fasta_bytes(recs, 60, b"\r\n")
    files["fq_no_final_newline"] = fastq_bytes(recs)[:-1]
    files["fa_no_final_newline"] = fasta_bytes(recs, 60)[:-1]
    files["fq_cr_last_byte"] = fastq_bytes(recs, 0, b"\r\n")[:-1]                  # the quality string ends in '\r' and the file with it
    files["fa_cr_alone_last_byte"] = fasta_bytes(recs, 60) + b"\r"                 # a line that is the file's last byte keeps its '\r'
    files["fa_upper_only"] = fasta_bytes(rand_records(13, b"ACGTN"), 60)
    # quality lines that start with '@' and with '+', one line each and wrapped
    q = [[b"q0", b"ACGTACGTAC", b"@IIIIIIII+"], [b"q1 c", b"acgtacgtac", b"+IIII@IIII"], [b"q2", b"A", b"@"], [b"q3", b"C", b"+"]]
    files["fq_at_plus"] = fastq_bytes(q)
    files["fq_at_plus_w5"] = fastq_bytes(q + [[b"q4", b"ACGTAACGTA", b"IIIII@IIII"], [b"q5", b"ACGTAACGTA", b"IIIII+IIII"]], 5)
    files["junk_in_front"] = b"no header here\n\n" + fasta_bytes(recs[:5], 60)
    files["empty_lines"] = b">a\n\nAC\n\nGT\n\n>b\n\n\n>c\nA\n"
    return files


def all_chunks(lib, path, **kw):
    """-> [(records, n_seqs, n_bases)] of FileChunks(path, **kw)"""
    return [(ch.records(), ns, nb) for ch, ns, nb in chunkpass.FileChunks(path, lib=lib, **kw)]


def check_file(lib, path, data=None):
    data = file_bytes(path) if data is None else data
    assert len(data) % 16384 != 0
    records, _, _ = kseq_records(data)
    for up in (True, False):
        got = all_chunks(lib, path, is_upper=up)
        assert len(got) == 1 and got[0][1] == len(records) and got[0][2] == sum(len(r[1]) for r in records)
        want = as_reads(records, up)
        if got[0][0] != want:
            bad = [i for i, (g, w) in enumerate(zip(got[0][0], want)) if g != w]
            raise AssertionError("%s, is_upper=%s: %d records against %d, first difference at %s: %r != %r" % (
                path, up, len(got[0][0]), len(want), bad[:1], got[0][0][bad[0]] if bad else None, want[bad[0]] if bad else None))
    return records


# ---- 1. gather parity ----
def check_gather_parity(lib, tmp_path, monkeypatch):
    for fn in ("tiny_all.fq.gz", "adv_all.fa.gz", "adv_sub.fq.gz", "adv_sub.fa.gz"):
        assert len(check_file(lib, os.path.join(GOLDEN, fn))) > 0
    files = seeded_files()
    src_res, dst_res, lower = set(), set(), False
    for name, data in files.items():
        plain, gz = str(tmp_path / name), str(tmp_path / (name + ".gz"))
        open(plain, "wb").write(data)
        with gzip.open(gz, "wb") as f:
            f.write(data)
        records = check_file(lib, plain, data)
        check_file(lib, gz, data)
        _, src, dst = kseq_records(data)
        src_res |= {s % 16 for s in src}                             # (one piece, one chunk: a line's offset in the file is its offset on the device)
        dst_res |= {d % 16 for d in dst}
        lower |= any(r[1] != r[1].upper() for r in records)
        if name == "fa_cr_alone_last_byte":
            assert records[-1][1].endswith(b"\r")
        if name == "fq_cr_last_byte":
            assert not records[-1][2].endswith(b"\r") and data.endswith(b"\r")
    assert src_res == set(range(16)) and dst_res == set(range(16)) and lower
    assert any(len(r[1]) == 0 for r in kseq_records(files["fq"])[0]) and any(len(r[1]) == 0 for r in kseq_records(files["fa_w60"])[0])
    # pieces shorter than a record, and than a line: records carried over, the piece grown
    for piece in ("16", "100", "4096"):
        monkeypatch.setenv("LQREADER_PIECE_BYTES", piece)
        for name in ("fq", "fa_w60", "fq_w7", "fa_crlf_w60", "fa_cr_alone_last_byte", "fq_cr_last_byte", "junk_in_front", "fq_at_plus_w5"):
            check_file(lib, str(tmp_path / name), files[name])
        check_file(lib, str(tmp_path / "fq_w60.gz"), files["fq_w60"])
    monkeypatch.delenv("LQREADER_PIECE_BYTES")
    # the packed layout of a file chunk is lqcov_pack_reads' on the same records, and the steps see the same chunk
    for name in ("fq", "fa_w17"):
        reads = as_reads(kseq_records(files[name])[0])
        for ch, _, _ in chunkpass.FileChunks(str(tmp_path / name), lib=lib):
            codes, amb, flags = ch.get_packed()
            w_codes, w_amb, w_flags = TC.host_pack(lib, [r[1] for r in reads])
            assert codes.tobytes() == w_codes.tobytes() and amb.tobytes() == w_amb.tobytes() and flags.tobytes() == w_flags.tobytes()
            assert flags.any() and len(ch) == len(reads) and ch.names == [r[0] for r in reads]
            assert ch.records([3, 4, 9, 2]) == [reads[i] for i in (3, 4, 9, 2)]
            other = chunkpass.ReadChunk(reads, lib=lib)
            for g, w in zip(ch.sdust(), other.sdust()):
                assert g[:ch.n].tobytes() == w[:ch.n].tobytes()
            other.close()


# ---- 2. reference pin ----
def check_reference_pin(lib, tmp_path):
    for fn, exp in (("tiny_all.fq.gz", "tiny_all.sdust.gz"), ("adv_sub.fq.gz", "adv_sub.sdust.gz")):
        lm = sdust.LqMaskMI355X(str(tmp_path / fn), lib=lib)
        n_chunks = 0
        for ch, _, _ in chunkpass.FileChunks(os.path.join(GOLDEN, fn), chunk_size=10000, is_upper=False, lib=lib):
            lm.submit_sdust(None, n_chunks, chunk=ch)
            n_chunks += 1
        lm.close_pool()
        assert n_chunks >= 2                                         # (rows of several chunks, in submission order)
        assert open(lm.get_outfile_path(), "rb").read() == gzip.open(os.path.join(GOLDEN, exp), "rb").read()
    records, _, _ = kseq_records(file_bytes(os.path.join(GOLDEN, "adv_all.fa.gz")))
    arr = lambda b: np.frombuffer(b, dtype=np.uint8)
    want = sdust.sdust_rows([r[0].decode() for r in records], [arr(r[1]) for r in records], [arr(b"!" * len(r[1])) for r in records], lib=lib)
    got = []
    for ch, _, _ in chunkpass.FileChunks(os.path.join(GOLDEN, "adv_all.fa.gz"), is_upper=False, lib=lib):
        got += sdust.sdust_rows(ch.names, None, None, chunk=ch)
    assert got == want and len(got) == len(records)


# ---- 3. chunk rule ----
def rule_records():
    rng = random.Random(5)
    return [[("read_%d" % i).encode() + b"x" * (i % 7), bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 120))), None] for i in range(330)]


def check_chunk_rule(lib, tmp_path):
    records = rule_records()
    path = str(tmp_path / "rule.fq")
    open(path, "wb").write(fastq_bytes([[a, b, b"I" * len(b)] for a, b, _ in records]))
    empty = str(tmp_path / "empty.fa")
    open(empty, "wb").write(b"")
    reads = as_reads(kseq_records(open(path, "rb").read())[0])
    assert len(reads) == 330
    size = lambda ov, rs: sum(3 * ov + len(r[0]) + 2 * len(r[1]) for r in rs)
    borders = {}
    for ov in (49, 41):
        cases = [size(ov, reads) // 4 + 1,                          # >= 3 chunks and a partial last one
                 None,                                              # the cumulative size at the last record: a trailing empty chunk
                 1, 0, 0.5]                                         # below one record: one read per chunk
        cases[1] = size(ov, reads)
        for cs in cases:
            want = ref_chunks(reads, cs, ov)
            got = all_chunks(lib, path, chunk_size=cs, str_overhead=ov)
            assert [(len(c), ns, nb) for c, ns, nb in got] == [(len(c), ns, nb) for c, ns, nb in want], (ov, cs)
            assert [c for c, _, _ in got] == [c for c, _, _ in want]
            ns = [x[1] for x in got]
            assert ns == sorted(ns) and ns[-1] == 330 and got[-1][2] == sum(len(r[1]) for r in reads)      # cumulative, never reset
            if cs == cases[0]:
                assert len(got) >= 3 and got[-1][0] and size(ov, got[-1][0]) < cs <= size(ov, got[0][0])      # a partial last chunk
                borders[ov] = ns
            if cs == cases[1]:
                assert len(got) == 2 and got[-1][0] == [] and len(got[0][0]) == 330                         # the trailing empty chunk is yielded
            if cs in (1, 0, 0.5):
                assert len(got) == 331 and all(len(c) == 1 for c, _, _ in got[:-1]) and got[-1][0] == []
        got = all_chunks(lib, empty, chunk_size=1000, str_overhead=ov)
        assert got == [([], 0, 0)]                                  # an empty file: one empty chunk
    # one chunk size for both overheads: the smaller overhead ends a chunk later
    cs = size(49, reads) // 4 + 1
    a = [x[1] for x in all_chunks(lib, path, chunk_size=cs, str_overhead=49)]
    b = [x[1] for x in all_chunks(lib, path, chunk_size=cs, str_overhead=41)]
    assert a != b and a == [x[1] for x in ref_chunks(reads, cs, 49)] and b == [x[1] for x in ref_chunks(reads, cs, 41)]
    # the default is the running interpreter's
    import sys
    assert chunkpass.FileChunks(path, lib=lib).str_overhead == sys.getsizeof("")


# ---- 4. drop-in parity ----
ADP5, ADP3 = sampleqc.PRESET_ADAPTERS["ont-ligation"]


def passes_equal(lib, tmp_path, path, cs, nsample, inds, gc_draw, tag, want_trim_hits=False, coverage=True):
    """run_file(path) against add_chunk(reads) on the test parser's records cut at the same borders -> the two passes"""
    reads = as_reads(kseq_records(open(path, "rb").read())[0])
    chunks = [c for c, _, _ in ref_chunks(reads, cs, 49)]
    assert len(chunks) >= 3 and sum(map(len, chunks)) == len(reads) > nsample
    kw = dict(adp5=ADP5, adp3=ADP3, nsample=nsample, inds=inds, gc_draw=gc_draw, gc_seed=3, suffix="x", lib=lib)
    a = chunkpass.SampleQCPass(str(tmp_path / (tag + "a")), "ont-ligation", **kw)
    np.random.seed(11)
    got = a.run_file(path, chunk_size=cs, trim=True, str_overhead=49)
    b = chunkpass.SampleQCPass(str(tmp_path / (tag + "b")), "ont-ligation", **kw)
    np.random.seed(11)
    want, want_trimmed = [], []
    for c in chunks:
        want.append(b.add_chunk(c))
        want_trimmed.append(b.trimmed)
    assert got == want[:len(got)] and len(got) == len(chunks)
    assert a.trimmed_chunks == want_trimmed
    if want_trim_hits:
        assert sum(t[0][1] for t in want) > 0 and sum(t[1][1] for t in want) > 0                # reads were trimmed at both ends
        assert any(x != y for t, c in zip(want_trimmed, chunks) for x, y in zip(t, c))
    # without trim the tuples are the same and no record is made
    c = chunkpass.SampleQCPass(str(tmp_path / (tag + "c")), "ont-ligation", **kw)
    np.random.seed(11)
    assert c.run_file(path, chunk_size=cs, str_overhead=49) == want and c.trimmed is None and c.trimmed_chunks == []
    for p in (a, b, c):
        p.mask.close_pool()
    table = open(b.mask.get_outfile_path(), "rb").read()
    assert open(a.mask.get_outfile_path(), "rb").read() == table == open(c.mask.get_outfile_path(), "rb").read() and table.count(b"\n") == len(reads)
    assert a.adapters.json_block() == b.adapters.json_block() == c.adapters.json_block()
    assert a.gc.json_block() == b.gc.json_block() and a.gc.gc_stats() == b.gc.gc_stats()
    assert a.gc.r_frac.tobytes() == b.gc.r_frac.tobytes() and a.gc.c_frac.tobytes() == b.gc.c_frac.tobytes() and len(a.gc.c_frac) > 0
    assert a.s_reads == b.s_reads == c.s_reads and len(a.s_reads) == nsample and all(a.s_reads)
    assert (a.cum_n_seq, a.chunk_n, a.n_bases) == (b.cum_n_seq, b.chunk_n, b.n_bases)
    c.close()
    return a, b, chunks


def check_drop_in(lib, tmp_path):
    T, _ = synth.make_dataset(synth.CONFIGS["tiny"])
    path = str(tmp_path / "tiny.fq")
    synth.write_fastq(path, T)
    cs, nsample, inds = 150000, 20, 100000
    for draw in ("device", "numpy"):
        a, b, chunks = passes_equal(lib, tmp_path, path, cs, nsample, inds, draw, draw)
        if draw == "numpy":
            a.close(); b.close()
            continue
        TC.assert_borders_interleave(chunks, inds)                   # index parts cross chunk borders and chunk borders cross parts
        # a reservoir replacement in a chunk after the one that fills the reservoir (lq_utils.py:371-411 restated for the check)
        first = np.cumsum([0] + [len(c) for c in chunks])
        fills = int(np.searchsorted(first, nsample, side="left")) - 1
        later = False
        for k in range(fills + 1, len(chunks)):
            u = np.random.RandomState(7).uniform(size=len(chunks[k]) + 1)[:len(chunks[k])]
            nth = first[k] + 1 + np.arange(len(chunks[k]))
            later |= bool(((u * nth).astype(np.int64) < nsample).any())
        assert later
        text = a.coverage()
        assert text == b.coverage() and sum(1 for l in text.splitlines() if l.split("\t")[2] != "0") > 10
        pair = a.coverage(short_threshold=500)
        assert isinstance(pair, tuple) and pair == b.coverage(short_threshold=500)
        # replace_masked over the file read again
        masked = [a.s_reads[1][0], a.s_reads[7][0]]
        fc = chunkpass.FileChunks(path, chunk_size=cs, str_overhead=49, lib=lib)
        got = a.coverage(exclude_seqs=masked, chunks=fc)
        want = b.coverage(exclude_seqs=masked, chunks=[(c, len(c), 0) for c in chunks])
        assert got == want and got != text
        swapped = sampleqc.replace_masked(a.s_reads, masked, fc)    # (the same FileChunks, iterated once more)
        assert swapped == sampleqc.replace_masked(b.s_reads, masked, [(c, len(c), 0) for c in chunks])
        assert len(swapped) == nsample and not {r[0] for r in swapped} & set(masked)
        a.close(); b.close()
    # reads with the adapters at their ends (test_chunkpass.step_reads), lower case in between: trimming and upper-casing
    seqs = TC.step_reads(9, 60)
    recs = TC.recs([s if i % 4 else s.lower() for i, s in enumerate(seqs)])
    path = str(tmp_path / "adapters.fq")
    open(path, "wb").write(fastq_bytes([[r[0].encode(), r[1].encode(), r[2].encode()] for r in recs], 80))
    a, b, _ = passes_equal(lib, tmp_path, path, 60000, 25, 4000000000, "device", "adp", want_trim_hits=True)
    a.close(); b.close()


# ---- 5. errors ----
def check_errors(lib, tmp_path):
    L = chunkpass._lib(lib)
    with pytest.raises(api.LqcovError) as e:
        list(chunkpass.FileChunks(str(tmp_path / "no_such_file.fq"), lib=lib))
    assert e.value.code == -2 and "no_such_file.fq" in str(e.value)
    assert b"no_such_file.fq" in L.lqreader_last_error(None)
    bad = str(tmp_path / "name.fq")
    open(bad, "wb").write(b"@ok\nACGT\n+\nIIII\n@caf\xc3\xa9\nACGT\n+\nIIII\n")
    with pytest.raises(api.LqcovError) as e:
        list(chunkpass.FileChunks(bad, lib=lib))
    assert e.value.code == -5 and "0x80" in str(e.value)
    # the message of a failing call through the handle, and nothing more from a reader that failed
    r = L.lqreader_open(bad.encode(), 0, 1 << 30, 1, 49, 0)
    ch = chunkpass.ReadChunk(None, lib=lib)
    import ctypes as C
    n, a, b, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
    args = (r, ch.h, C.byref(n), C.byref(a), C.byref(b), C.byref(last))
    assert L.lqreader_next(*args) == -5 and b"0x80" in L.lqreader_last_error(r)
    assert L.lqreader_next(*args) == -4 and L.lqreader_last_error(r)
    L.lqreader_close(r)
    ch.close()
    # a short quality string in the last record: the records before it, then the end
    cut = str(tmp_path / "cut.fq")
    open(cut, "wb").write(b"@a\nACGT\n+\nIIII\n@b\nAC\nGT\n+\nII\nII\n@c\nACGTACGT\n+\nIIII\n")
    for cs in (1 << 30, 1):
        got = all_chunks(lib, cut, chunk_size=cs)
        assert [r for c, _, _ in got for r in c] == [["a", "ACGT", "IIII"], ["b", "ACGT", "IIII"]] and got[-1][1:] == (2, 8)
        assert len(got) == (1 if cs > 1 else 3)
    assert kseq_records(open(cut, "rb").read())[0] == [[b"a", b"ACGT", b"IIII"], [b"b", b"ACGT", b"IIII"]]
    # a chunk from a file refuses what a chunk refuses
    for ch, _, _ in chunkpass.FileChunks(cut, lib=lib):
        idx, buf = np.array([5], dtype=np.uint32), np.zeros(64, np.uint8)
        assert L.lqchunk_get_reads(ch.h, 1, idx.ctypes.data, buf.ctypes.data, None) == -1 and b"outside" in L.lqchunk_last_error(ch.h)


# ---- the emulator build ----
def test_emulated_file_chunks_equal_the_parsed_records(emu_lib, tmp_path, monkeypatch):
    check_gather_parity(emu_lib, tmp_path, monkeypatch)


def test_emulated_file_chunks_give_the_reference_sdust_table(emu_lib, tmp_path):
    check_reference_pin(emu_lib, tmp_path)


def test_emulated_chunk_rule(emu_lib, tmp_path):
    check_chunk_rule(emu_lib, tmp_path)


def test_emulated_run_file_equals_add_chunk(emu_lib, tmp_path):
    check_drop_in(emu_lib, tmp_path)


def test_emulated_reader_errors(emu_lib, tmp_path):
    check_errors(emu_lib, tmp_path)


def test_the_restated_kseq_reads_the_goldens_as_the_reference_did():
    """kseq_records against what the reference binary printed for the same files (name and length of every record)"""
    for fn, exp in (("tiny_all.fq.gz", "tiny_all.sdust.gz"), ("adv_sub.fq.gz", "adv_sub.sdust.gz"), ("adv_all.fa.gz", "adv_all.sdust.gz")):
        records, _, _ = kseq_records(file_bytes(os.path.join(GOLDEN, fn)))
        rows = [l.split("\t") for l in read_gz(exp).splitlines()]
        assert [(r[0].decode(), str(len(r[1]))) for r in records] == [(x[0], x[2]) for x in rows]


# ---- the gfx950 build ----
@pytest.mark.gpu
def test_gpu_file_chunks_equal_the_parsed_records(gpu_lib, tmp_path, monkeypatch):
    check_gather_parity(gpu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_file_chunks_give_the_reference_sdust_table(gpu_lib, tmp_path):
    check_reference_pin(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_chunk_rule(gpu_lib, tmp_path):
    check_chunk_rule(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_run_file_equals_add_chunk(gpu_lib, tmp_path):
    check_drop_in(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_reader_errors(gpu_lib, tmp_path):
    check_errors(gpu_lib, tmp_path)

"""One upload per chunk (longqc_amd/chunkpass.py over lqchunk_* / lqstore_*, chunk.cpp, kernels_chunk.hpp), under the wave emulator
and on the GPU:
  1. k_chunk_pack writes the bytes lqcov_pack_reads writes on the host, and the flags of lqcov_packed_ambiguous_reads;
  2. lqchunk_sdust / _adapt / _gc return the arrays of lqsdust_reads / lqadapt_reads / lqgc_reads, with the same argument errors,
     also for a second, larger chunk in the same handle;
  3. SampleQCPass.coverage() returns the text of sampleqc.coverage_in_memory on the same reads -- and the committed golden table
     of the tiny input in 100-kbase parts -- with part borders inside chunks and chunk borders inside parts;
  4. what add_chunk leaves behind (sdust table, adapter tuples and trimmed records, GC_stats, subsample) is what the separate
     modules leave when called as INTEGRATION.md shows them."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from longqc_amd import adapter, api, chunkpass, gcfrac, sampleqc, sdust, synth
from tests.conftest import GOLDEN, read_gz
from tests.helpers import read_fastx


# ---- inputs ----
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def put(s, at, c):
    return s[:at] + c + s[at + 1:]


def pack_reads(seed, ambiguous=True):
    """check 1's reads: the edge lengths, several thousand bases, either case, U and u, N and other IUPAC letters at the first and
    the last base and at word (32) and chunk (128) borders, raw 0..3 -- or, ambiguous=False, none of that but the cases and U"""
    rng = random.Random(seed)
    clean = "ACGTacgtUu"
    seqs = [rand_seq(rng, l, clean) for l in (0, 1, 31, 32, 33, 127, 128, 129, 4000, 5123, 0, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257)]
    seqs += [rand_seq(rng, rng.randint(1, 300), clean) for _ in range(120)]
    if not ambiguous:
        return seqs
    for l in (1, 31, 32, 33, 127, 128, 129, 700, 3000):
        s = rand_seq(rng, l, clean)
        seqs.append(put(s, 0, "N"))
        seqs.append(put(s, l - 1, "n"))
        for at in (31, 32, 33, 127, 128, 129, 2047, 2048):
            if at < l:
                seqs.append(put(s, at, rng.choice("NRYKMSWBDHVnrykmswbdhv-*E")))
    seqs.append("\x00\x01\x02\x03" * 40 + "ACGT")                 # seq_nt4_table: the raw values are themselves
    seqs.append("".join(chr(c) for c in range(4, 256) if chr(c) not in "ACGTUacgtu"))   # every other byte is ambiguous
    seqs.append(rand_seq(rng, 6000, "ACGTN"))
    rng.shuffle(seqs)
    return seqs


def recs(seqs, qual=True, as_bytes=False, prefix="r"):
    out = []
    for i, s in enumerate(seqs):
        q = "".join(chr(33 + (7 * i + j) % 60) for j in range(len(s)))
        r = ["%s%d" % (prefix, i), s.encode("latin-1") if as_bytes else s]
        if qual:
            r.append(q.encode() if as_bytes else q)
        out.append(r)
    return out


def flat_of(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return "".join(seqs).encode("latin-1"), off


# ---- 1. pack parity ----
def host_pack(lib, seqs):
    flat, off = flat_of(seqs)
    n = len(seqs)
    nc = int(lib.lqcov_packed_chunks(n, off.ctypes.data))
    codes, amb, flags = np.zeros(max(nc, 1) * 4, np.uint64), np.zeros(max(nc, 1) * 4, np.uint32), np.zeros(max(n, 1), np.uint8)
    assert lib.lqcov_pack_reads(n, flat, off.ctypes.data, codes.ctypes.data, amb.ctypes.data, 1) == 0
    lens = np.diff(off).astype(np.uint32)
    assert lib.lqcov_packed_ambiguous_reads(n, amb.ctypes.data, lens.ctypes.data, flags.ctypes.data) == 0
    return codes[:nc * 4], amb[:nc * 4], flags[:n]


def check_pack(lib, seqs, want_ambiguous):
    _, off = flat_of(seqs)
    assert set(int(o) % 16 for o in off[:-1]) == set(range(16))       # the reads start at every residue mod 16 of the buffer
    ch = chunkpass.ReadChunk(recs(seqs, qual=False), lib=lib)
    codes, amb, flags = ch.get_packed()
    w_codes, w_amb, w_flags = host_pack(lib, seqs)
    assert codes.tobytes() == w_codes.tobytes()
    assert amb.tobytes() == w_amb.tobytes()
    assert flags.tobytes() == w_flags.tobytes()
    assert bool(flags.any()) == want_ambiguous
    ch.close()


def check_pack_parity(lib):
    check_pack(lib, pack_reads(1), True)
    check_pack(lib, pack_reads(2, ambiguous=False), False)        # a chunk without an ambiguous base
    T, _ = synth.make_dataset(synth.CONFIGS["tiny"])
    seqs = [s.tobytes().decode() for s in T.seqs]
    check_pack(lib, seqs, any("N" in s for s in seqs))
    # an empty chunk, and one of empty reads only
    for seqs in ([], ["", ""]):
        ch = chunkpass.ReadChunk(recs(seqs, qual=False), lib=lib)
        codes, amb, flags = ch.get_packed()
        assert codes.shape == (0,) and amb.shape == (0,) and not flags.any()
        ch.close()


# ---- 2. step parity ----
def raw_sdust(lib, seqs, quals, W=64, T=20):
    lib = sdust._lib(lib)
    flat, off = flat_of(seqs)
    n = len(seqs)
    qflat = "".join(quals).encode("latin-1") if quals else None
    o = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint32)
    err = C.create_string_buffer(512)
    rc = lib.lqsdust_reads(0, n, flat, off.ctypes.data, qflat, W, T, o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data, err, 512)
    return rc, err.value.decode(), o


def raw_adapt(lib, seqs, a5, a3, length):
    lib = adapter._lib(lib)
    flat, off = flat_of(seqs)
    n = len(seqs)
    o5, o3 = np.zeros((max(n, 1), 4), np.int32), np.zeros((max(n, 1), 4), np.int32)
    err = C.create_string_buffer(512)
    rc = lib.lqadapt_reads(0, n, flat, off.ctypes.data, a5, len(a5) if a5 else 0, a3, len(a3) if a3 else 0, length,
                           o5.ctypes.data, o3.ctypes.data, err, 512)
    return rc, err.value.decode(), o5[:n], o3[:n]


ADP5, ADP3 = (a.encode() for a in sampleqc.PRESET_ADAPTERS["ont-ligation"])


def step_reads(seed, n_long):
    rng = random.Random(seed)
    seqs = [rand_seq(rng, l) for l in (1, 149, 150, 299, 300, 301, 750, 751)]
    seqs += [rand_seq(rng, rng.randint(1, 40)) for _ in range(50)]
    seqs += [rand_seq(rng, rng.randint(300, 3000), "ACGTACGTACGTN") for _ in range(n_long)]
    seqs.append("AT" * 600 + rand_seq(rng, 500) + "A" * 400)       # low complexity
    for i in range(0, n_long, 3):                                  # adapters at some ends, with an error or two
        s = seqs[58 + i]
        a5, a3 = ADP5.decode(), ADP3.decode()
        seqs[58 + i] = rand_seq(rng, 7) + put(a5, 5, "A") + s + (a3 if i % 2 else put(a3, 3, "T")) + rand_seq(rng, 4)
    rng.shuffle(seqs)
    return seqs


def check_steps_on(lib, ch, seqs, with_qual):
    n = len(seqs)
    quals = [r[2] for r in recs(seqs)] if with_qual else None
    # sdust
    for W, T in ((64, 20), (16, 10)):
        rc, _, want = raw_sdust(lib, seqs, quals, W, T)
        assert rc == 0
        got = ch.sdust(W, T)
        for g, w in zip(got, want):
            assert g[:n].tobytes() == w[:n].tobytes()
    assert got[0][:n].any()
    # adapters
    for a5, a3, length in ((ADP5, ADP3, 150), (ADP5, None, 150), (None, ADP3, 60), (b"ACGT" * 30, ADP3, 150)):
        rc, _, w5, w3 = raw_adapt(lib, seqs, a5, a3, length)
        assert rc == 0
        g5, g3 = ch.adapt(a5, a3, length)
        assert (g5 is None) == (a5 is None) and (g3 is None) == (a3 is None)
        if a5:
            assert g5.tobytes() == w5.tobytes()
        if a3:
            assert g3.tobytes() == w3.tobytes()
    assert (g3[:, 0] >= 0).any()
    # GC: no draws, the device's draw, positions given (the numpy draw's path)
    flat, off = flat_of(seqs)
    lens = np.diff(off).astype(np.int64)
    k = gcfrac.draws_per_read(lens, 150, 0.2).astype(np.uint32)
    np.random.seed(5)
    pos_in = np.concatenate([np.random.choice(int(l), int(kk), replace=False) for l, kk in zip(lens, k)]).astype(np.uint32)
    for kk, pp, seed, first in ((None, None, 0, 0), (k, None, 77, 12345), (k, pos_in, 0, 0)):
        want = gcfrac._call(lib, 0, flat, off, 150, kk, pp, seed, first)
        got = gcfrac._call(lib, 0, None, None, 150, kk, pp, seed, first, chunk=ch)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert g.tobytes() == w.tobytes()
    assert got[2].any() and want[0].any()


def errors_of(lib, ch, seqs):
    """(code, message) of the argument errors, from the chunk and from the buffer-level calls"""
    L = ch.lib
    n = len(seqs)
    flat, off = flat_of(seqs)
    o = np.zeros(4 * n + 4, np.uint32)
    p = o.ctypes.data
    out = []

    def both(rc_chunk, raw):
        out.append(((rc_chunk, L.lqchunk_last_error(ch.h).decode()), (raw[0], raw[1])))
    both(L.lqchunk_sdust(ch.h, 2, 20, p, p, p), raw_sdust(lib, seqs, None, W=2))
    both(L.lqchunk_sdust(ch.h, 67, 20, p, p, p), raw_sdust(lib, seqs, None, W=67))
    both(L.lqchunk_adapt(ch.h, ADP5, len(ADP5), None, 0, 0, p, p), raw_adapt(lib, seqs, ADP5, None, 0))
    both(L.lqchunk_adapt(ch.h, ADP5, len(ADP5), None, 0, 4097, p, p), raw_adapt(lib, seqs, ADP5, None, 4097))
    both(L.lqchunk_adapt(ch.h, ADP5, 32769, None, 0, 150, p, p), (lambda r: r)(_raw_adapt_len(lib, seqs, 32769)))
    g = gcfrac._lib(lib)
    err = C.create_string_buffer(512)

    def raw_gc(cs, k, doff, pos, gc_p=p, kept_p=p, win_p=p):
        a = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)
        k_, d_, p_ = a(k, np.uint32), a(doff, np.uint64), a(pos, np.uint32)
        q = lambda v: None if v is None else v.ctypes.data
        rc = g.lqgc_reads(0, n, flat, off.ctypes.data, cs, q(k_), q(d_), q(p_), 0, 0, gc_p, None, win_p, kept_p, err, 512)
        rc2 = L.lqchunk_gc(ch.h, cs, q(k_), q(d_), q(p_), 0, 0, gc_p, None, win_p, kept_p)
        out.append(((rc2, L.lqchunk_last_error(ch.h).decode()), (rc, err.value.decode())))
    zeros = [0] * n
    raw_gc(0, None, None, None)
    raw_gc(4097, None, None, None)
    raw_gc(150, None, None, None, gc_p=None)
    raw_gc(150, zeros, None, None)
    raw_gc(150, [len(seqs[0]) + 1] + zeros[1:], [0] + [len(seqs[0]) + 1] * n, None)       # more draws than bases
    raw_gc(150, [1] + zeros[1:], [0] + [2] * n, None)                                     # draw_off is not k's prefix sum
    raw_gc(150, [1] + zeros[1:], [0] + [1] * n, [len(seqs[0])])                           # a position outside its read
    raw_gc(150, [1] + zeros[1:], [0] + [1] * n, [0], win_p=None)
    return out


def _raw_adapt_len(lib, seqs, len5):
    lib = adapter._lib(lib)
    flat, off = flat_of(seqs)
    o = np.zeros((len(seqs) + 1, 4), np.int32)
    err = C.create_string_buffer(512)
    rc = lib.lqadapt_reads(0, len(seqs), flat, off.ctypes.data, ADP5, len5, None, 0, 150, o.ctypes.data, o.ctypes.data, err, 512)
    return rc, err.value.decode()


def check_step_parity(lib):
    small, large = step_reads(3, 30), step_reads(4, 90)
    assert sum(map(len, large)) > 2 * sum(map(len, small))
    for with_qual in (True, False):
        ch = chunkpass.ReadChunk(recs(small, qual=with_qual), lib=lib)
        check_steps_on(lib, ch, small, with_qual)
        ch.load(recs(large, qual=with_qual, as_bytes=True))         # a second, larger chunk in the same handle: the buffers grow
        check_steps_on(lib, ch, large, with_qual)
        ch.load(recs(small, qual=with_qual))                        # and a smaller one in the grown buffers
        check_steps_on(lib, ch, small, with_qual)
        ch.close()
    ch = chunkpass.ReadChunk(recs(small, qual=False), lib=lib)
    errs = errors_of(lib, ch, small)
    assert len(errs) == 13
    for got, want in errs:
        assert got == want and got[0] in (-1, -5) and got[1], (got, want)
    assert [g[0] for g, _ in errs] == [-5, -5, -5, -5, -5, -5, -5, -1, -1, -1, -1, -1, -1]
    # state errors of the handle itself
    L = ch.lib
    assert L.lqchunk_get_packed(ch.h, None, None, None) == -4
    off = np.array([0, 5, 3], dtype=np.uint64)
    assert L.lqchunk_load(ch.h, 2, b"ACGTACGT", off.ctypes.data, None) == -1 and "ascending" in L.lqchunk_last_error(ch.h).decode()
    o = np.zeros(8, np.uint32)
    assert L.lqchunk_sdust(ch.h, 64, 20, o.ctypes.data, o.ctypes.data, o.ctypes.data) == -4       # the failed load left no chunk
    ch.close()


# ---- 3. table parity ----
def tiny_chunks(chunk_reads=37, edit=None):
    n, s, q = read_fastx(os.path.join(GOLDEN, "tiny_all.fq.gz"))
    reads = [[a, b.tobytes().decode(), c.tobytes().decode()] for a, b, c in zip(n, s, q)]
    if edit:
        reads = edit(reads)
    return [reads[i:i + chunk_reads] for i in range(0, len(reads), chunk_reads)]


def tiny_queries():
    n, s, q = read_fastx(os.path.join(GOLDEN, "tiny_sub.fq.gz"))
    return [[a, b.tobytes().decode(), c.tobytes().decode()] for a, b, c in zip(n, s, q)]


def part_borders(lens, batch, mini=50000000):
    """the first read of every index part after the first, by the reference's rule (index.c:244,311-316) restated"""
    mini = min(mini, batch)
    out, part_bases, pend = [], 0, 0
    for i, l in enumerate(lens):
        if pend == 0 and i and part_bases > batch:
            out.append(i)
            part_bases = 0
        pend += l
        if pend >= mini:
            part_bases += pend
            pend = 0
    return out


def assert_borders_interleave(chunks, batch):
    lens = [len(r[1]) for c in chunks for r in c]
    parts = part_borders(lens, batch)
    cuts = list(np.cumsum([len(c) for c in chunks])[:-1])
    assert len(parts) + 1 >= 3 and len(cuts) + 1 >= 3
    assert not set(parts) & set(cuts)
    edges = sorted([(p, "part") for p in parts] + [(c, "chunk") for c in cuts])
    kinds = [k for _, k in edges]
    assert any(a != b for a, b in zip(kinds, kinds[1:]))             # a part border inside a chunk and a chunk border inside a part
    for c0, c1 in zip([0] + cuts, cuts + [len(lens)]):
        if any(c0 < p < c1 for p in parts):
            break
    else:
        raise AssertionError("no part border inside a chunk")
    for p0, p1 in zip([0] + parts, parts + [len(lens)]):
        if any(p0 < c < p1 for c in cuts):
            break
    else:
        raise AssertionError("no chunk border inside a part")
    return parts


def run_pass(lib, tmp_path, chunks, s_reads, **kw):
    sp = chunkpass.SampleQCPass(str(tmp_path), "ont-ligation", inds=100000, lib=lib)
    for c in chunks:
        sp.add_chunk(c)
    assert sp.store.nbytes > 0
    text = sp.coverage(s_reads=s_reads, **kw)
    sp.close()
    return text


def run_in_memory(lib, chunks, s_reads, **kw):
    p, _, _ = api.parse_args(sampleqc.coverage_argv("ont-ligation", "x", "y", inds="100000"))
    eng = api.Engine(p, 0, lib=lib)
    text = sampleqc.coverage_in_memory([(c, len(c), 0) for c in chunks], s_reads, inds=100000, engine=eng, **kw)
    eng.close()
    return text


def check_table_parity(lib, tmp_path):
    chunks, s_reads = tiny_chunks(), tiny_queries()
    assert_borders_interleave(chunks, 100000)
    text = run_pass(lib, tmp_path, chunks, s_reads, out=str(tmp_path / "cov.txt"))
    assert text == read_gz("tiny_parts.table.gz")                   # the committed golden table of this input in 100-kbase parts
    assert text == run_in_memory(lib, chunks, s_reads) and open(str(tmp_path / "cov.txt")).read() == text
    # two sets in one pass
    both = run_pass(lib, tmp_path, chunks, s_reads, short_threshold=500)
    assert isinstance(both, tuple) and len(both) == 2 and both == run_in_memory(lib, chunks, s_reads, short_threshold=500)
    cut = sorted(len(r[1]) for r in s_reads)[len(s_reads) // 3] + 1     # (and a threshold that leaves reads on both sides)
    both = run_pass(lib, tmp_path, chunks, s_reads, short_threshold=cut)
    assert both[0] and both[1] and both == run_in_memory(lib, chunks, s_reads, short_threshold=cut)

    # an N-bearing read in one part only: the other parts go to the engine without ambiguity words
    def one_n(reads):
        lens = [len(r[1]) for r in reads]
        parts = part_borders(lens, 100000)
        for r in reads:
            r[1] = "".join(c if c in "ACGT" else "A" for c in r[1])
        at = parts[0] + 1
        assert at < parts[1]
        reads[at][1] = put(reads[at][1], len(reads[at][1]) // 2, "N")
        return reads
    chunks = tiny_chunks(edit=one_n)
    parts = assert_borders_interleave(chunks, 100000)
    flat = [r for c in chunks for r in c]
    assert [i for i, r in enumerate(flat) if "N" in r[1]] == [parts[0] + 1]
    text = run_pass(lib, tmp_path, chunks, s_reads)
    assert text == run_in_memory(lib, chunks, s_reads)


# ---- 4. drop-in parity ----
def check_drop_in(lib, tmp_path):
    seqs = step_reads(9, 60)
    cut = [0, 40, 41, 90, len(seqs)]
    a5, a3 = ADP5.decode(), ADP3.decode()
    # the separate modules, as INTEGRATION.md shows them
    lm = sdust.LqMaskMI355X(str(tmp_path / "a"), "x", lib=lib)
    lg = gcfrac.LqGCMI355X(chunk_size=150, draw="device", seed=3, lib=lib)
    stats = adapter.AdapterStats(a5, a3)
    s_reads, cum, want_results, want_trimmed = [], 0, [], []
    for n, (a, b) in enumerate(zip(cut, cut[1:])):
        reads = recs(seqs[a:b], prefix="c%d_" % n)
        lm.submit_sdust(reads, n)
        copy = [list(r) for r in reads]
        want_results.append(adapter.cut_adapter(copy, adp_t=a5, adp_b=a3, lib=lib))
        stats.add(want_results[-1])
        want_trimmed.append(copy)
        s_reads = sampleqc.subsample_from_chunk(reads, cum, s_reads, 25)
        lg.calc_read_and_chunk_gc_frac(reads)
        cum += len(reads)
    lm.close_pool()
    # one pass
    sp = chunkpass.SampleQCPass(str(tmp_path / "b"), "ont-ligation", adp5=a5, adp3=a3, nsample=25, gc_seed=3, suffix="x", lib=lib)
    for n, (a, b) in enumerate(zip(cut, cut[1:])):
        reads = recs(seqs[a:b], prefix="c%d_" % n)
        keep = [list(r) for r in reads]
        assert sp.add_chunk(reads) == want_results[n]
        assert sp.trimmed == want_trimmed[n] and reads == keep       # the caller's records stay untrimmed
    sp.mask.close_pool()
    assert want_results[0][0][1] > 0 and want_results[0][1][1] > 0  # reads were trimmed at both ends
    assert open(sp.mask.get_outfile_path()).read() == open(lm.get_outfile_path()).read()
    assert os.path.basename(sp.mask.get_outfile_path()) == "longqc_sdust_x.txt"
    assert sp.adapters.json_block() == stats.json_block() and stats.json_block()
    assert sp.gc.json_block() == lg.json_block()
    assert sp.gc.r_frac.tobytes() == lg.r_frac.tobytes() and sp.gc.c_frac.tobytes() == lg.c_frac.tobytes()
    assert (sp.gc.r_tot, sp.gc.c_tot, sp.gc.r_gc_tot, sp.gc.c_gc_tot) == (lg.r_tot, lg.c_tot, lg.r_gc_tot, lg.c_gc_tot)
    assert sp.s_reads == s_reads and sp.cum_n_seq == cum and len(s_reads) == 25
    sp.close()
    # cut_adapter with chunk= trims the records it is given, like cut_adapter without
    reads = recs(seqs[:40])
    ch = chunkpass.ReadChunk(reads, lib=lib)
    ll_a, ll_b = [1], [1]
    got = adapter.cut_adapter(reads, len_list=ll_a, adp_t=a5, adp_b=a3, chunk=ch)
    other = recs(seqs[:40])
    assert got == adapter.cut_adapter(other, len_list=ll_b, adp_t=a5, adp_b=a3, lib=lib) and reads == other and ll_a == ll_b
    ch.close()
    # the two ways the reference's GC loop raises, on a chunk
    bad = recs(["ACGT" * 300, "", "ACGT" * 200], qual=False)
    for draw in ("device", "numpy"):
        a, b = gcfrac.LqGCMI355X(draw=draw, lib=lib), gcfrac.LqGCMI355X(draw=draw, lib=lib)
        ch = chunkpass.ReadChunk(bad, lib=lib)
        np.random.seed(2)
        with pytest.raises(ZeroDivisionError):
            a.calc_read_and_chunk_gc_frac(bad, chunk=ch)
        np.random.seed(2)
        with pytest.raises(ZeroDivisionError):
            b.calc_read_and_chunk_gc_frac(bad)
        assert a.r_frac.tobytes() == b.r_frac.tobytes() and a.c_frac.tobytes() == b.c_frac.tobytes() and a.n_reads == b.n_reads == 1
        with pytest.raises(ValueError):
            a.calc_read_and_chunk_gc_frac(bad, samp_rate=200, chunk=ch)
        with pytest.raises(ValueError):
            b.calc_read_and_chunk_gc_frac(bad, samp_rate=200)
        assert a.r_frac.tobytes() == b.r_frac.tobytes() and a.r_tot == b.r_tot
        ch.close()


# ---- the emulator build ----
def test_emulated_pack_equals_the_host_pack(emu_lib):
    check_pack_parity(emu_lib)


def test_emulated_steps_equal_the_buffer_level_calls(emu_lib):
    check_step_parity(emu_lib)


def test_emulated_tables_equal_the_in_memory_path(emu_lib, tmp_path):
    check_table_parity(emu_lib, tmp_path)


def test_emulated_chunk_loop_equals_the_separate_modules(emu_lib, tmp_path):
    check_drop_in(emu_lib, tmp_path)


# ---- the gfx950 build ----
@pytest.mark.gpu
def test_gpu_pack_equals_the_host_pack(gpu_lib):
    check_pack_parity(gpu_lib)
    fr = synth.make_reads_flat(synth.CONFIGS["cfg1"])              # 1000 reads ~10 kb: every lane shape of k_chunk_pack's tiles
    flat = fr.flat.tobytes().decode("latin-1")
    check_pack(gpu_lib, [flat[int(fr.off[i]):int(fr.off[i + 1])] for i in range(len(fr))] + pack_reads(7), True)


@pytest.mark.gpu
def test_gpu_steps_equal_the_buffer_level_calls(gpu_lib):
    check_step_parity(gpu_lib)


@pytest.mark.gpu
def test_gpu_tables_equal_the_in_memory_path(gpu_lib, tmp_path):
    check_table_parity(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_chunk_loop_equals_the_separate_modules(gpu_lib, tmp_path):
    check_drop_in(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_cfg1_in_one_mbase_parts(gpu_lib, tmp_path):
    """BASELINE configs[0] (1000 ONT reads ~10 kb, every read a query) in chunks of 97 reads and parts of 1 Mbase: the pass and the
    in-memory path give the same table"""
    T, Q = synth.make_dataset(synth.CONFIGS["cfg1"])
    to = lambda rs: [[n, s.tobytes().decode(), q.tobytes().decode()] for n, s, q in zip(rs.names, rs.seqs, rs.quals)]
    reads, s_reads = to(T), to(Q)
    chunks = [reads[i:i + 97] for i in range(0, len(reads), 97)]
    assert_borders_interleave(chunks, 1000000)
    sp = chunkpass.SampleQCPass(str(tmp_path), "ont-ligation", inds=1000000, lib=gpu_lib)
    for c in chunks:
        sp.add_chunk(c)
    text = sp.coverage(s_reads=s_reads)
    sp.close()
    assert text == sampleqc.coverage_in_memory([(c, len(c), 0) for c in chunks], s_reads, inds=1000000)
    assert sum(1 for l in text.splitlines() if l.split("\t")[2] != "0") > 100

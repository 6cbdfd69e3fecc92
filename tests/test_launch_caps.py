"""The chunk-step kernels past their launch caps.  k_chunk_pack, k_sdust, k_adapt, k_gc_reads, k_gc_draw and k_gc_windows cap their
grid and stride their work list over the launch; a real chunk makes every one of them run its loop several times per thread.  Each
check here is the smallest input that reaches the second round of one kernel -- the loop increment, the partial last tile, what a
thread carries from one item to the next, the atomics on gc[] and kept[] -- against a reference written in numpy (or the oracle's
`sdust`, or test_adapter's restated edlib), under the wave emulator and on the GPU.

The caps are read from the kernel headers; every check asserts that its shape exceeds the cap, that at least 100 items fall into the
second round and that the last tile / block / group of the launch is partial: a raised cap fails the test instead of emptying it."""
import glob
import os
import random
import re
import subprocess
import time

import numpy as np
import pytest

from longqc_amd import chunkpass, sdust
from longqc_amd import gcfrac as G
from tests import oracle_bind
from tests import test_adapter as TA
from tests import test_chunkpass as TC
from tests import test_gcfrac as TG
from tests import test_sdust as SD
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "longqc_amd", "csrc")


def header_define(name):
    """the integer a kernel header gives `name` in a #define line"""
    for fn in sorted(glob.glob(os.path.join(CSRC, "kernels_*.hpp"))):
        m = re.search(r"^#define\s+%s\s+(\d+)[uU]?\b" % re.escape(name), open(fn).read(), re.M)
        if m:
            return int(m.group(1))
    raise AssertionError("no #define %s in longqc_amd/csrc/kernels_*.hpp" % name)


def assert_past_cap(what, n_items, per_round, last_unit=None):
    """the three conditions of every check: more items than one round of the launch takes, at least 100 of them in the second
    round, and a partial last unit (n_items is no multiple of `last_unit`; None: the caller asserts it in its own units)"""
    assert n_items > per_round, "%s: %d items do not exceed the %d a launch takes in its first round (cap raised?)" % (what, n_items, per_round)
    assert n_items - per_round >= 100, "%s: only %d items in the second round" % (what, n_items - per_round)
    assert last_unit is None or n_items % last_unit != 0, "%s: %d items fill the last unit of %d" % (what, n_items, last_unit)


def timed(label, t0):
    print("%s: %.2f s" % (label, time.time() - t0))


# ---- 1. k_chunk_pack ----------------------------------------------------------------------------------------------------
CLEAN = np.frombuffer(b"ACGTacgtUu", dtype=np.uint8)
RAW = np.arange(4, dtype=np.uint8)                                  # seq_nt4_table: the values 0..3 are themselves
OTHER = np.frombuffer(b"NRYKMSWBDHVnrykmswbdhv-*E@\x04\x7f\xff", dtype=np.uint8)
EDGES = (0, 1, 30, 31, 32, 33, 63, 64, 95, 96, 126, 127, 128, 129, 255, 256)


def pack_input(ambiguous, seed):
    """-> (flat uint8, lens int64).  One-chunk reads (1..128 bases) in runs far longer than a tile, empty reads at random, at tile
    borders and at the end, a few hundred reads of 129..700 bases, two of 5000 and more that straddle a tile border (one per
    round); other bytes at the first and the last base and around the word and chunk borders of reads of both rounds"""
    tile, cap = header_define("LQ_PACK_TILE_CHUNKS"), header_define("LQ_PACK_MAX_BLOCKS")
    rng = np.random.default_rng(seed)
    n = (cap + 101) * tile + 37
    lens = rng.integers(1, 129, n)
    lens[rng.choice(n, 300, replace=False)] = rng.integers(129, 701, 300)
    lens[n - 1 - rng.choice(6000, 100, replace=False)] = rng.integers(129, 701, 100)      # (enough of them in the second round)
    lens[rng.choice(n, 400, replace=False)] = 0
    lens[1000:1080] = rng.integers(1, 129, 80)                      # (a run of one-chunk reads whatever the draws above did)
    lens[n - 3000:n - 2920] = rng.integers(1, 129, 80)
    # the two long reads: where the chunk count so far leaves fewer than their chunks in the tile
    for lo, l in ((5000, 5003), (n - 2000, 6500)):
        coff = np.concatenate([[0], np.cumsum((lens + 127) // 128)])
        r = lo + int(np.flatnonzero(coff[lo:lo + 200] % tile > tile // 2)[0])
        lens[r] = l
    # empty reads where a tile begins (the tile's first chunk is then the read's after them), in both rounds; and as the last reads
    coff = np.concatenate([[0], np.cumsum((lens + 127) // 128)])
    first = np.flatnonzero((coff[:-1] % tile == 0) & (lens > 0))
    at = np.concatenate([first[5:400:7], first[first > n - 5000][::5]])
    lens = np.insert(lens, at, 0)
    lens[-1] = 50
    lens = np.concatenate([lens, [0, 0, 0]])
    if ((lens + 127) // 128).sum() % tile == 0:
        lens = np.concatenate([lens[:-3], [77, 0, 0, 0]])
    n = lens.shape[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = CLEAN[rng.integers(0, CLEAN.shape[0], int(off[n]))]
    # other bytes: every long read, 3000 reads anywhere and 1500 of the last 6000 reads
    special = np.unique(np.concatenate([np.flatnonzero(lens > 128), rng.choice(n, 3000, replace=False), n - 1 - rng.choice(6000, 1500, replace=False)]))
    for e in EDGES + (-1,):
        rs = special[lens[special] > (e if e >= 0 else 0)]
        rs = rs[rng.random(rs.shape[0]) < 0.5]
        other = ambiguous & (rng.random(rs.shape[0]) < 0.5)
        flat[off[rs] + (e if e >= 0 else lens[rs] - 1)] = np.where(other, OTHER[rng.integers(0, OTHER.shape[0], rs.shape[0])], RAW[rng.integers(0, 4, rs.shape[0])])
    if ambiguous:                                                  # and reads that are nothing but other bytes, one per round
        for r in (int(np.flatnonzero(lens > 200)[3]), int(np.flatnonzero(lens > 200)[-3])):
            flat[off[r]:off[r + 1]] = OTHER[rng.integers(0, OTHER.shape[0], int(lens[r]))]
    return flat, lens


def numpy_pack(flat, lens):
    """the layout at the top of kernels_chunk.hpp, restated: every read starts on a chunk of 128 bases = 4 words of 32; a base is
    seq_nt4_table's code (either case, U as T, the raw values 0..3 as themselves, 4 for everything else), base j of a word at bits
    2j..2j+1 of the u64 (0 where ambiguous) and bit j of the u32 set where it is ambiguous or lies behind the read's end"""
    nt4 = np.full(256, 4, dtype=np.uint8)
    for c, letters in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
        nt4[list(letters)] = c
    nt4[:4] = np.arange(4)
    n = lens.shape[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    coff = np.concatenate([[0], np.cumsum((lens + 127) // 128)])
    slot = np.full(int(coff[n]) * 128, 4, dtype=np.uint8)           # behind a read's end: ambiguous
    code = nt4[flat]
    slot[np.repeat(coff[:-1] * 128 - off[:-1], lens) + np.arange(flat.shape[0])] = code
    slot = slot.reshape(-1, 32)
    bad = slot == 4
    sh = np.arange(32, dtype=np.uint64)
    codes = (np.where(bad, 0, slot).astype(np.uint64) << (2 * sh)).sum(axis=1, dtype=np.uint64)
    amb = (bad.astype(np.uint32) << sh.astype(np.uint32)).sum(axis=1, dtype=np.uint32)
    nbad = np.concatenate([[0], np.cumsum(code == 4)])
    flags = (nbad[off[1:]] > nbad[off[:-1]]).astype(np.uint8)
    return codes, amb, flags


def check_pack_past_cap(lib, ambiguous):
    tile, cap = header_define("LQ_PACK_TILE_CHUNKS"), header_define("LQ_PACK_MAX_BLOCKS")
    t0 = time.time()
    flat, lens = pack_input(ambiguous, seed=31 if ambiguous else 32)
    n = lens.shape[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    coff = np.concatenate([[0], np.cumsum((lens + 127) // 128)])
    n_chunks = int(coff[n])
    assert_past_cap("k_chunk_pack, packed chunks", n_chunks, cap * tile, tile)
    assert (n_chunks + tile - 1) // tile - cap >= 100               # whole tiles of the second round
    # the shape: what the kernel's work list looks like for this input
    tile_read = np.minimum(np.searchsorted(coff, np.arange((n_chunks + tile - 1) // tile + 1) * tile, side="right") - 1, n - 1)
    span = np.diff(tile_read)
    assert (span[:cap] == tile).any() and (span[cap:] == tile).any()            # tiles of 64 one-chunk reads: the bisect over 65 entries
    assert (span[:cap] > tile).any() and (span[cap:] > tile).any()              # and over more, with empty reads in between
    begins = (coff[:-1] % tile == 0) & (coff[:-1] < n_chunks)
    assert (begins & (lens == 0))[coff[:-1] < cap * tile].any() and (begins & (lens == 0))[coff[:-1] >= cap * tile].any()
    assert (lens[-3:] == 0).all() and lens[-4] > 0
    long_ = np.flatnonzero(lens >= 5000)
    assert long_.shape[0] == 2 and coff[long_[0] + 1] < cap * tile <= coff[long_[1]]
    assert (coff[long_] // tile != (coff[long_ + 1] - 1) // tile).all()         # both straddle a tile border
    assert ((lens > 128) & (lens <= 700)).sum() >= 250
    assert set((off[:-1][lens > 0] % 16).tolist()) == set(range(16))
    second = coff[:-1] >= cap * tile                                            # reads whose tiles lie at or past the cap
    for e in EDGES + (-1,):                                                     # raw and other bytes at every edge, in both rounds
        for rs in (np.flatnonzero(~second & (lens > max(e, 0))), np.flatnonzero(second & (lens > max(e, 0)))):
            there = flat[off[rs] + (e if e >= 0 else lens[rs] - 1)]
            assert (there < 4).any() and np.isin(there, OTHER).any() == ambiguous, e
    seqs = flat.tobytes().decode("latin-1")
    reads = [["r", seqs[a:b]] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    timed("pack input (%d reads, %d bases, %d chunks, %d tiles)" % (n, off[n], n_chunks, tile_read.shape[0] - 1), t0)
    t0 = time.time()
    ch = chunkpass.ReadChunk(reads, lib=lib)
    codes, amb, flags = ch.get_packed()
    ch.close()
    timed("ReadChunk + get_packed", t0)
    t0 = time.time()
    w_codes, w_amb, w_flags = TC.host_pack(lib, [r[1] for r in reads])          # (a) the project's host packer
    n_codes, n_amb, n_flags = numpy_pack(flat, lens)                            # (b) the layout restated
    timed("references", t0)
    assert n_codes.tobytes() == w_codes.tobytes() and n_amb.tobytes() == w_amb.tobytes() and n_flags.tobytes() == w_flags.tobytes()
    for got, want, what in ((codes, n_codes, "codes"), (amb, n_amb, "amb"), (flags, n_flags, "flags")):
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero(got != want) if got.shape == want.shape else None
            raise AssertionError("%s differ: shapes %s / %s, first at %s of %d (words of the second round start at %d)"
                                 % (what, got.shape, want.shape, None if bad is None else bad[:5], got.shape[0], cap * tile * 4))
    if ambiguous:
        assert flags[~second].any() and flags[second].any() and not flags.all()
    else:
        assert not flags.any()                                                  # no ambiguous base: every flag zero


# ---- 2. k_sdust ---------------------------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_PAIRS = 200                                                       # reads r < N_PAIRS are paired with read r + cap on purpose


def sdust_input(seed):
    """-> (flat, lens, qual): cap + ~3000 reads of 0..120 bases (a few of 300..2000 in both rounds) made of random sequence,
    tandem repeats of unit 1..3 at 3 % substitutions and two-letter random stretches, with N runs and lower case.  Thread t walks
    read t and then read t + cap: for t < N_PAIRS read t is a clean tandem repeat and read t + cap is, by t % 4, another repeat /
    one or two bases / empty / a read that begins with N"""
    cap = header_define("LQ_DUST_MAX_THREADS")
    rng = np.random.default_rng(seed)
    n = cap + 3000 + 21
    lens = rng.integers(0, 121, n)
    lens[rng.choice(np.arange(N_PAIRS, cap), 6, replace=False)] = rng.integers(300, 2001, 6)
    lens[rng.choice(np.arange(cap + N_PAIRS, n), 6, replace=False)] = rng.integers(300, 2001, 6)
    # per half of a read: 0 random, 1 tandem repeat, 2 two random letters.  The reference's list of perfect intervals makes a clean
    # repeat cost the oracle the square of its length and two-letter sequence a fifth of that: both are common in the reads of
    # the threads that walk two reads (masking is what a thread's leftovers would change) and rare in the others, which fill the launch
    two_reads = (np.arange(n) < n - cap) | (np.arange(n) >= cap)
    mode = np.where(two_reads[:, None], rng.choice(3, (n, 2), p=[0.4, 0.15, 0.45]), rng.choice(3, (n, 2), p=[0.97, 0.01, 0.02]))
    ulen = rng.integers(1, 4, (n, 2))
    unit = rng.integers(0, 4, (n, 2, 3))
    pair = np.stack([rng.integers(0, 4, n), rng.integers(0, 4, n)], axis=1)
    noise = np.full(n, 0.03)
    a = np.arange(N_PAIRS)
    b = a + cap
    lens[a] = rng.integers(40, 121, N_PAIRS)
    mode[a] = 1; ulen[a] = 1 + (a[:, None] // 4) % 3; noise[a] = 0  # strongly low-complexity, the same unit in both halves
    unit[a, 1] = unit[a, 0]
    kind = a % 4
    k0, k1, k2, k3 = (b[kind == i] for i in range(4))
    lens[k0] = rng.integers(40, 121, k0.shape[0])
    mode[k0] = 1; ulen[k0] = 2 + (k0[:, None] // 4) % 2; noise[k0] = 0
    for j in range(3):                                              # a unit of other letters than read r's
        unit[k0, :, j] = (unit[k0 - cap, 0, 0][:, None] + 1 + j) % 4
    lens[k1] = 1 + (k1 // 4) % 2
    lens[k2] = 0
    lens[k3] = rng.integers(5, 121, k3.shape[0])
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[n])
    rid = np.repeat(np.arange(n), lens)
    j = np.arange(total) - off[rid]
    half = (j >= rng.integers(0, lens + 1)[rid]).astype(np.int64)
    m = mode[rid, half]
    rnd = rng.integers(0, 4, total)
    code = np.where(m == 0, rnd, np.where(m == 1, unit[rid, half, j % ulen[rid, half]], pair[rid, rng.integers(0, 2, total)]))
    code = np.where((m == 1) & (rng.random(total) < noise[rid]), rnd, code)
    flat = ACGT[code]
    free = np.ones(n, bool); free[a] = False                        # (the paired first reads stay clean)
    with_n = free & (rng.random(n) < 0.08) & (lens >= 4)
    s = rng.integers(0, np.maximum(lens, 1)); e = s + rng.integers(1, 5, n)
    flat[with_n[rid] & (j >= s[rid]) & (j < e[rid])] = ord("N")
    lower = free & (rng.random(n) < 0.1)
    s = rng.integers(0, np.maximum(lens, 1)); e = s + rng.integers(1, 60, n)
    flat[lower[rid] & (j >= s[rid]) & (j < e[rid])] |= 0x20
    flat[off[k3]] = ord("N")
    qual = (33 + rng.integers(2, 45, total)).astype(np.uint8)
    return flat, lens, qual


def write_fastx(path, names, flat, off, qual=None):
    s, q = flat.tobytes().decode(), (qual.tobytes().decode() if qual is not None else None)
    with open(path, "w") as f:
        for i, nm in enumerate(names):
            a, b = int(off[i]), int(off[i + 1])
            f.write("@%s\n%s\n+\n%s\n" % (nm, s[a:b], q[a:b]) if q is not None else ">%s\n%s\n" % (nm, s[a:b]))


def check_sdust_past_cap(lib, tmp_path, pin_reference):
    cap, block = header_define("LQ_DUST_MAX_THREADS"), header_define("LQ_DUST_THREADS")
    t0 = time.time()
    flat, lens, qual = sdust_input(seed=41)
    n = lens.shape[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    assert_past_cap("k_sdust, reads", n, cap, block)
    assert ((lens[:cap] >= 300).sum() >= 6) and ((lens[cap:] >= 300).sum() >= 6)
    a = np.arange(N_PAIRS); b = a + cap
    first = flat[off[:-1][lens > 0]]
    assert (lens[a] >= 40).all() and (lens[b[a % 4 == 1]] < 3).all() and (lens[b[a % 4 == 1]] > 0).all() and (lens[b[a % 4 == 2]] == 0).all()
    assert (flat[off[b[a % 4 == 3]]] == ord("N")).all() and (first == ord("N")).sum() >= N_PAIRS // 4
    assert (flat == ord("N")).sum() > 1000 and ((flat & 0x20) != 0).sum() > 10000
    names = ["s%d" % i for i in range(n)]
    seqs = [flat[x:y] for x, y in zip(off[:-1].tolist(), off[1:].tolist())]
    quals = [qual[x:y] for x, y in zip(off[:-1].tolist(), off[1:].tolist())]
    s = flat.tobytes().decode(); q = qual.tobytes().decode()
    fq, fa = str(tmp_path / "caps.fq"), str(tmp_path / "caps.fa")
    write_fastx(fq, names, flat, off, qual)
    write_fastx(fa, names, flat, off)
    timed("sdust input (%d reads, %d bases)" % (n, off[n]), t0)
    exe = oracle_bind.ensure_oracle()
    ref = os.path.join(os.path.dirname(oracle_bind.REF_BIN), "sdust")
    # W/T 64/20 on the reads with quality strings, 16/10 on the same reads without
    for W, T, path, with_q in ((64, 20, fq, True), (16, 10, fa, False)):
        t0 = time.time()
        opts = ["-w", str(W), "-t", str(T)]
        want = subprocess.run([exe, "sdust"] + opts + [path], stdout=subprocess.PIPE, check=True).stdout.decode()
        if pin_reference and os.path.exists(ref):                    # the oracle's table for this input is the reference binary's
            assert subprocess.run([ref] + opts + [path], stdout=subprocess.PIPE, check=True).stdout.decode() == want
        rows = want.splitlines()
        assert len(rows) == n
        masked = np.array([int(r.split("\t")[1]) for r in rows])
        print("W=%d T=%d: %d of %d bases masked, %d of %d reads of the second round with masked bases" % (W, T, masked.sum(), off[n], (masked[cap:] > 0).sum(), n - cap))
        two_reads = (np.arange(n) < n - cap) | (np.arange(n) >= cap)
        assert masked[two_reads].sum() > 0.3 * lens[two_reads].sum() and (masked[cap:] > 0).sum() > 1000 and (masked[b[a % 4 == 0]] > 0).all()
        timed("oracle", t0)
        t0 = time.time()
        got = sdust.sdust_rows(names, seqs, quals if with_q else None, w=W, t=T, lib=lib)
        first_diff(got, rows, cap, "sdust_rows W=%d T=%d" % (W, T))
        reads = [[nm, s[x:y], q[x:y]] if with_q else [nm, s[x:y]] for nm, x, y in zip(names, off[:-1].tolist(), off[1:].tolist())]
        ch = chunkpass.ReadChunk(reads, lib=lib)                      # the resident path
        got = sdust.sdust_rows(names, None, None, w=W, t=T, chunk=ch)
        ch.close()
        first_diff(got, rows, cap, "ReadChunk.sdust W=%d T=%d" % (W, T))
        rc, out, err = SD.run_sdust_main(lib, opts + [path], tmp=tmp_path)      # one mini-batch: the same strided launch
        assert rc == 0, err
        first_diff(out.splitlines(), rows, cap, "lqsdust_main W=%d T=%d" % (W, T))
        assert out == want
        timed("three paths", t0)


def first_diff(got, want, cap, what):
    if got != want:
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        raise AssertionError("%s: %d rows against %d, %d differ, %d of them in the first round; first: %r != %r"
                             % (what, len(got), len(want), len(bad), sum(1 for i in bad if i < cap), got[bad[0]] if bad else None, want[bad[0]] if bad else None))


# ---- 3. k_adapt ---------------------------------------------------------------------------------------------------------
def edited(adp, n_edits, prng):
    a = list(adp)
    for _ in range(n_edits):
        p, op = prng.randrange(len(a)), prng.randrange(3)
        if op == 0:
            a[p] = prng.choice("ACGT")
        elif op == 1:
            a.insert(p, prng.choice("ACGT"))
        else:
            del a[p]
    return "".join(a)


def adapt_input(adp5, adp3, length, lo, hi, seed):
    """cap + ~150 reads of lo..hi >= 2 * length bases with 500 shorter ones in between (some among the last 150), the adapters
    with 0..3 edits at both ends of every third eligible read"""
    cap = header_define("LQ_ADAPT_MAX_BLOCKS")
    rng, prng = np.random.default_rng(seed), random.Random(seed)
    n = cap + 157 + 500
    short = np.zeros(n, bool)
    short[rng.choice(n - 150, 480, replace=False)] = True
    short[n - 150 + rng.choice(150, 20, replace=False)] = True
    lens = np.where(short, rng.integers(0, 2 * length, n), rng.integers(lo, hi + 1, n))
    lens[np.flatnonzero(short)[::9]] = 2 * length - 1
    lens[np.flatnonzero(~short)[::11]] = 2 * length
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = ACGT[rng.integers(0, 4, int(off[n]))].tobytes().decode()
    seqs = [flat[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    planted = np.flatnonzero(~short)[::3]
    for rank, i in enumerate(planted.tolist()):
        s = TA.implant(seqs[i], edited(adp5, rank % 4, prng), prng, 0.0, 5, prng.randrange(4))
        seqs[i] = TA.implant(s, edited(adp3, (rank // 4) % 4, prng), prng, 0.0, 3, prng.randrange(4))
        assert len(seqs[i]) == lens[i]
    return seqs, planted


def check_adapt_past_cap(lib, banded, n_first=150):
    cap = header_define("LQ_ADAPT_MAX_BLOCKS")
    rng = random.Random(7)
    t0 = time.time()
    if banded:
        adp5, adp3, length, lo, hi = TA.rand_seq(rng, 66), TA.rand_seq(rng, 70), 40, 80, 130
    else:
        adp5, adp3, length, lo, hi = TA.rand_seq(rng, 12), TA.rand_seq(rng, 12), 24, 48, 90
    assert (len(adp5) > 64) == (len(adp3) > 64) == banded          # k_adapt<true> / k_adapt<false> for both adapters
    seqs, planted = adapt_input(adp5, adp3, length, lo, hi, seed=51 + banded)
    lens = np.array([len(s) for s in seqs])
    elig = np.flatnonzero(lens >= 2 * length)                       # the launch's ends, in this order
    assert_past_cap("k_adapt, read ends per adapter", elig.shape[0], cap, cap)
    second, firsts = elig[cap:], elig[:cap]
    assert (lens < 2 * length).sum() == 500 and (np.flatnonzero(lens < 2 * length) > second[0]).sum() >= 10     # the scatter back is no identity
    assert np.isin(second, planted).sum() >= second.shape[0] // 3
    assert "LQADAPT_BATCH_READS" not in os.environ                  # one launch per adapter
    timed("adapter input (%d reads, %d bases)" % (len(seqs), lens.sum()), t0)
    t0 = time.time()
    rc, o5, o3, err = TA.call_reads(lib, seqs, adp5, adp3, length)
    assert rc == 0, err
    timed("lqadapt_reads", t0)
    t0 = time.time()
    assert (o5[lens < 2 * length] == -1).all() and (o3[lens < 2 * length] == -1).all()
    assert (o5[elig, 0] >= 0).all() and (o3[elig, 0] >= 0).all()
    sample = np.sort(np.random.default_rng(3).choice(firsts, n_first, replace=False))      # n_first reads = 2 * n_first ends
    for rows, what in ((second, "second round"), (sample, "first round")):
        sub = [seqs[i] for i in rows.tolist()]
        for o, adp, which in ((o5, adp5, 5), (o3, adp3, 3)):
            want = TA.hits_want(sub, adp, length, which)
            np.testing.assert_array_equal(o[rows], want, err_msg="%s, %d' ends (d, s, e, L)" % (what, which))
            if what == "second round":                              # implants lie there (a short read's two implants overlap)
                p = np.isin(rows, planted)
                assert p.sum() >= rows.shape[0] // 3 and (want[p, 0] <= max(0, len(adp) - length) + 6).sum() >= p.sum() // 6
    timed("restated edlib on %d + %d ends" % (2 * second.shape[0], 2 * n_first), t0)


# ---- 4. the GC kernels --------------------------------------------------------------------------------------------------
def gc_reference(flat, off, cs, k=None, pos=None):
    """-> (gc, win, kept) from the prefix sums of (byte == 'G') | (byte == 'C'): the count of window i is P[min(i + cs, l)] - P[i],
    kept the first draw j with i + cs - 1 > l (k where there is none), counts at or after kept zero"""
    P = np.concatenate([[0], np.cumsum((flat == ord("G")) | (flat == ord("C")))]).astype(np.int64)
    off = off.astype(np.int64)
    gc = (P[off[1:]] - P[off[:-1]]).astype(np.uint32)
    if k is None:
        return gc, None, None
    k = np.asarray(k, dtype=np.int64)
    n = k.shape[0]
    r = np.repeat(np.arange(n), k)
    j = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)
    i = np.asarray(pos, dtype=np.int64)
    l = (off[1:] - off[:-1])[r]
    win = P[off[r] + np.minimum(i + cs, l)] - P[off[r] + i]
    kept = k.copy()
    np.minimum.at(kept, r, np.where(i + cs - 1 > l, j, k[r]))
    win[j >= kept[r]] = 0
    return gc, win.astype(np.uint16), kept.astype(np.uint32)


def test_the_vectorised_gc_reference_equals_the_walk():
    """gc_reference against walk() of test_gcfrac.py on 200 reads, at window sizes on both sides of the read lengths"""
    rng = np.random.default_rng(61)
    lens = rng.integers(1, 900, 200)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = np.frombuffer(b"ACGTacgtNS", dtype=np.uint8)[rng.integers(0, 10, int(off[-1]))]
    k = np.minimum(lens, rng.integers(0, 12, 200))
    pos = np.concatenate([rng.choice(int(l), int(kk), replace=False) for l, kk in zip(lens, k)])
    doff = np.concatenate([[0], np.cumsum(k)])
    for cs in (1, 64, 150, 4096):
        gc, win, kept = gc_reference(flat, off, cs, k, pos)
        stopped = 0
        for r in range(200):
            seq = flat[off[r]:off[r + 1]].tobytes()
            want_kept, counts = TG.walk(seq, [int(p) for p in pos[doff[r]:doff[r + 1]]], cs)
            assert kept[r] == want_kept and list(win[doff[r]:doff[r] + want_kept]) == counts and not win[doff[r] + want_kept:doff[r + 1]].any()
            assert gc[r] == seq.count(b"G") + seq.count(b"C")
            stopped += want_kept < k[r]
        assert (0 < stopped < 200) or cs in (1, 4096)


def gc_call(lib, flat, off, cs, k=None, pos_in=None, seed=0, first=0):
    return G._call(lib, 0, flat.tobytes(), off.astype(np.uint64), cs, k, pos_in, seed, first)


def check_gc_windows_past_cap(lib, monkeypatch):
    cap, per_block = header_define("LQ_GC_MAX_BLOCKS"), header_define("LQ_GC_THREADS") // 16
    rng = np.random.default_rng(71)
    lens = rng.integers(400, 3001, 300)
    lens[[20, 140, 250, 297]] = rng.integers(9000, 12001, 4)        # reads that hold whole windows of 4096
    n = lens.shape[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = np.frombuffer(b"ACGTacgtNS", dtype=np.uint8)[rng.integers(0, 10, int(off[n]))]
    k = lens // 13
    k[-1] -= int(k.sum() % per_block == 0)
    nd = int(k.sum())
    doff = np.concatenate([[0], np.cumsum(k)])
    assert_past_cap("k_gc_windows, draws", nd, cap * per_block, per_block)
    assert off[n] < (128 << 20) and "LQGC_BATCH_BASES" not in os.environ      # one span: the rounds are rounds of one launch
    second = np.arange(nd) >= cap * per_block
    for cs in (150, 4096):
        # positions given, np.random.choice's: every position of the read for a third of the reads (their walk stops early), for
        # the others those that stop no walk, where the read has as many
        st = np.random.RandomState(5)
        room = np.where((np.arange(n) % 3 == 0) | (lens - cs + 2 < k), lens, lens - cs + 2)
        given = np.concatenate([st.choice(int(m), int(kk), replace=False) for m, kk in zip(room, k)]).astype(np.uint32)
        for pos_in, seed in ((given, 0), (None, 77)):
            t0 = time.time()
            gc, pos, win, kept = gc_call(lib, flat, off, cs, k, pos_in, seed, 12345)
            want_pos = given if pos_in is not None else TG.ref_draw(seed, 12345, lens, k)
            assert (pos == want_pos).all()
            w_gc, w_win, w_kept = gc_reference(flat, off, cs, k, want_pos)
            for got, want, what in ((gc, w_gc, "gc"), (kept, w_kept, "kept"), (win, w_win, "win")):
                bad = np.flatnonzero(got != want)
                assert bad.shape[0] == 0, "%s, chunk_size %d, %s: %d differ, first at %s (draws of the second round start at %d): %s != %s" % (
                    what, cs, "positions given" if pos_in is not None else "device draw", bad.shape[0], bad[:5], cap * per_block, got[bad[:5]], want[bad[:5]])
            in_kept = (np.arange(nd) - np.repeat(doff[:-1], k)) < np.repeat(w_kept.astype(np.int64), k)
            print("chunk_size %d, %s: %d of %d draws before kept, %d of them in the second round" % (cs, "given" if pos_in is not None else "device", in_kept.sum(), nd, (in_kept & second).sum()))
            if pos_in is not None:
                assert (w_win[second] > 0).sum() >= 100 and (w_kept < k).any() and ((w_kept == k) & (k > 0)).any()
            monkeypatch.setenv("LQGC_BATCH_BASES", "65536")         # the same call in spans of 64 KiB: identical arrays
            again = gc_call(lib, flat, off, cs, k, pos_in, seed, 12345)
            monkeypatch.delenv("LQGC_BATCH_BASES")
            for a, b in zip((gc, pos, win, kept), again):
                assert a.tobytes() == b.tobytes()
            timed("k_gc_windows chunk_size %d" % cs, t0)


def check_gc_draw_past_cap(lib):
    cap, block = header_define("LQ_GC_MAX_BLOCKS"), header_define("LQ_GC_THREADS")
    full = 21001
    n_full = cap * block // full + 2                                # 26 reads drawn in full, and two more
    rng = np.random.default_rng(81)
    lens = np.full(n_full + 6, full)
    shorts = {0: 5, 7: 149, 8: 751, 15: 3000, n_full + 4: 1, n_full + 5: 150}
    for i, l in shorts.items():
        lens[i] = l
    n = lens.shape[0]
    k = np.where(lens == full, lens, G.draws_per_read(lens, 150, 0.2))
    k[0] = 5
    nd = int(k.sum())
    assert_past_cap("k_gc_draw, draws", nd, cap * block, block)
    off = np.concatenate([[0], np.cumsum(lens)])
    doff = np.concatenate([[0], np.cumsum(k)])
    flat = ACGT[rng.integers(0, 4, int(off[n]))]
    t0 = time.time()
    gc, pos, win, kept = gc_call(lib, flat, off, 150, k, None, 2 ** 64 - 3, 2 ** 40)
    timed("lqgc_reads, %d draws" % nd, t0)
    t0 = time.time()
    want_pos = TG.ref_draw(2 ** 64 - 3, 2 ** 40, lens, k)
    bad = np.flatnonzero(pos != want_pos)
    assert bad.shape[0] == 0, "pos: %d differ, first at %s (draws of the second round start at %d)" % (bad.shape[0], bad[:5], cap * block)
    for r in np.flatnonzero(k == lens).tolist():                    # a read drawn in full: a permutation of its positions
        assert (np.sort(pos[doff[r]:doff[r + 1]]) == np.arange(lens[r])).all(), r
    w_gc, w_win, w_kept = gc_reference(flat, off, 150, k, want_pos)
    assert (gc == w_gc).all() and (kept == w_kept).all() and (win == w_win).all()
    assert (w_kept < k).any() and w_win.any() and w_win[cap * block:].any()
    timed("reference", t0)


def check_gc_reads_past_cap(lib):
    cap, tile, waves = header_define("LQ_GC_MAX_BLOCKS"), header_define("LQ_GC_TILE"), header_define("LQ_GC_THREADS") // 64
    per_round = cap * waves                                         # tiles of the first round
    rng = np.random.default_rng(91)
    t0 = time.time()
    border = per_round * tile
    # the first round: reads of 1..6 Mbases; then a 2-Mbase read from 1 Mbase before the border, 600 short reads with empty ones
    # in between, a read of a few tiles and more short reads: the second round holds whole tiles inside one read, tiles over many
    # reads and empty reads
    head = []
    while sum(head) < border - (7 << 20):
        head.append(int(rng.integers(1 << 20, 6 << 20)))
    head.append(border - (1 << 20) - sum(head))
    short = rng.integers(5, 301, 1800)
    short[rng.choice(1800, 150, replace=False)] = 0
    lens = np.concatenate([head, [2 << 20], short[:600], [5 * tile + 123], short[600:], [0, 0]]).astype(np.int64)
    n = lens.shape[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[n])
    n_tiles = (total + tile - 1) // tile
    assert_past_cap("k_gc_reads, tiles", n_tiles, per_round)
    assert total % tile != 0                                        # the last tile is partial
    big = len(head)
    assert off[big] + tile < border and off[big + 1] > border + 100 * tile      # whole tiles of the second round inside one read
    in_second = off[:-1] >= border
    assert (in_second & (lens == 0)).sum() >= 100 and (in_second & (lens > 0) & (lens <= 300)).sum() >= 1500
    assert (off[:-1][in_second] // tile != (off[1:][in_second] - 1) // tile).sum() >= 30      # short reads over tile borders
    flat = np.frombuffer(b"ACGTacgtNGC", dtype=np.uint8)[rng.integers(0, 11, total)]
    isgc = ((flat == ord("G")) | (flat == ord("C"))).astype(np.uint32)
    want = np.zeros(n, dtype=np.uint32)
    want[lens > 0] = np.add.reduceat(isgc, off[:-1][lens > 0])
    timed("gc input (%d reads, %d bytes, %d tiles)" % (n, total, n_tiles), t0)
    t0 = time.time()
    gc, _, _, _ = gc_call(lib, flat, off, 150)
    timed("lqgc_reads", t0)
    bad = np.flatnonzero(gc != want)
    assert bad.shape[0] == 0, "gc: %d reads differ, first %s (read %d holds the border of the rounds): %s != %s" % (bad.shape[0], bad[:5], big, gc[bad[:5]], want[bad[:5]])
    assert want[in_second].sum() > 10000


# ---- the emulator build -------------------------------------------------------------------------------------------------
ORDERS = ["lowest", "reverse", "random:5"]                          # the emulator's thread orders (tests/emu/hipemu.hpp)


def set_order(monkeypatch, order):
    if order == "lowest":
        monkeypatch.delenv("LQ_EMU_ORDER", raising=False)
    else:
        monkeypatch.setenv("LQ_EMU_ORDER", order)


@pytest.mark.parametrize("order", ORDERS)
def test_emulated_pack_past_the_cap(emu_lib, monkeypatch, order):
    set_order(monkeypatch, order)
    check_pack_past_cap(emu_lib, ambiguous=True)


def test_emulated_pack_past_the_cap_without_ambiguous_bases(emu_lib):
    check_pack_past_cap(emu_lib, ambiguous=False)


def test_emulated_sdust_past_the_cap(emu_lib, tmp_path):
    check_sdust_past_cap(emu_lib, tmp_path, pin_reference=True)


def test_emulated_adapt_past_the_cap_plain(emu_lib):
    check_adapt_past_cap(emu_lib, banded=False)


def test_emulated_adapt_past_the_cap_banded(emu_lib):
    check_adapt_past_cap(emu_lib, banded=True)


@pytest.mark.parametrize("order", ORDERS)
def test_emulated_gc_windows_past_the_cap(emu_lib, monkeypatch, order):
    set_order(monkeypatch, order)
    check_gc_windows_past_cap(emu_lib, monkeypatch)


def test_emulated_gc_draw_past_the_cap(emu_lib):
    check_gc_draw_past_cap(emu_lib)


def test_emulated_gc_reads_past_the_cap(emu_lib):
    check_gc_reads_past_cap(emu_lib)


# ---- the gfx950 build ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pack_past_the_cap(gpu_lib):
    check_pack_past_cap(gpu_lib, ambiguous=True)


@pytest.mark.gpu
def test_gpu_pack_past_the_cap_without_ambiguous_bases(gpu_lib):
    check_pack_past_cap(gpu_lib, ambiguous=False)


@pytest.mark.gpu
def test_gpu_sdust_past_the_cap(gpu_lib, tmp_path):
    check_sdust_past_cap(gpu_lib, tmp_path, pin_reference=False)


@pytest.mark.gpu
def test_gpu_adapt_past_the_cap_plain(gpu_lib):
    check_adapt_past_cap(gpu_lib, banded=False)


@pytest.mark.gpu
def test_gpu_adapt_past_the_cap_banded(gpu_lib):
    check_adapt_past_cap(gpu_lib, banded=True)


@pytest.mark.gpu
def test_gpu_gc_windows_past_the_cap(gpu_lib, monkeypatch):
    check_gc_windows_past_cap(gpu_lib, monkeypatch)


@pytest.mark.gpu
def test_gpu_gc_draw_past_the_cap(gpu_lib):
    check_gc_draw_past_cap(gpu_lib)


@pytest.mark.gpu
def test_gpu_gc_reads_past_the_cap(gpu_lib):
    check_gc_reads_past_cap(gpu_lib)

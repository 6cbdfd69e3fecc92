"""k_bgzf_inflate (longqc_amd/csrc/kernels_inflate.hpp) through the array call lqinflate_blocks / chunkpass.inflate_blocks, under the
wave emulator and on the GPU.  The oracle is zlib: every expected byte is the payload the test compressed with zlib or, for the
streams of tests/deflate_writer.py, what zlib.decompress makes of them (checked here, without a GPU, before they are used).
  1. byte-exact output: random ACGT, FASTQ text, one repeated byte, repeats of period 2, 3, 5 and 67, random bytes; the sizes 0, 1, 2,
     257, 258, 259, 32768, 65279, 65280, 65535, 65536; levels 0, 1, 6, 9 crossed with the strategies default, Z_FIXED, Z_RLE and
     Z_HUFFMAN_ONLY; streams with a Z_SYNC_FLUSH and a Z_FULL_FLUSH in the middle; the writer's streams.  Many blocks per launch,
     output offsets at every residue mod 16, a guard pattern between the ranges.
     The cross: every payload kind at every size up to 259 with all 16 (level, strategy) pairs; at the five large sizes every kind
     with four of the pairs, rotated so that every pair meets every large size and every kind (the large sizes differ in where the
     last block ends, which no level or strategy changes; the emulator runs 64 fibers per member).  65536 bytes fit a BGZF member only
     when they compress; random bytes stop at 65280 (stored: 65290 bytes).
  2. corrupt streams, one bad block among good ones in one launch: the status class, the neighbours' bytes, the guards."""
import random
import zlib

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import deflate_writer as DW

SIZES = (0, 1, 2, 257, 258, 259, 32768, 65279, 65280, 65535, 65536)
LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY)
PAIRS = [(lv, st) for lv in LEVELS for st in STRATEGIES]
GUARD = 0xEE
INVALID = (chunkpass.INFLATE_INVALID, chunkpass.INFLATE_INPUT)
LENGTH = (chunkpass.INFLATE_LONG, chunkpass.INFLATE_SHORT)
MEMBER_MAX = 65536 - 26                                             # deflate bytes of the largest BGZF member


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, a = b"", 0
    for at, mode in flush_at:
        out += c.compress(data[a:at]) + c.flush(mode)
        a = at
    return out + c.compress(data[a:]) + c.flush()


def payloads(n, seed):
    """kind -> n bytes"""
    rng = random.Random(seed)
    fq = b"".join(b"@read%d/%d\n%s\n+\n%s\n" % (i, rng.randrange(9999), bytes(rng.choices(b"ACGT", k=rng.randint(50, 300))),
                                              bytes(rng.choices(b"!#(-5:?DIK", k=40))) for i in range(n // 150 + 2))
    out = {"acgt": bytes(rng.choices(b"ACGT", k=n)), "fastq": fq[:n], "one_byte": b"G" * n, "random": rng.randbytes(n)}
    for p in (2, 3, 5, 67):
        unit = rng.randbytes(p)
        out["period_%d" % p] = (unit * (n // p + 1))[:n]
    return out


def zlib_cases():
    """-> [(name, deflate bytes, payload)] -- made once per session"""
    if not hasattr(zlib_cases, "made"):
        cases, large = [], 0
        for n in SIZES:
            for k, (kind, data) in enumerate(sorted(payloads(n, 100 + n).items())):
                if n <= 259:
                    pairs = PAIRS
                else:                                               # four of the sixteen: pair p for (large + k + 4 j) mod 16 == p
                    pairs = [PAIRS[(large + k + 4 * j) % 16] for j in range(4)]
                for lv, st in pairs:
                    comp = raw_deflate(data, lv, st)
                    if len(comp) <= MEMBER_MAX:
                        cases.append(("%s_%d_l%d_s%d" % (kind, n, lv, st), comp, data))
            large += n > 259
        fq = payloads(40000, 7)["fastq"]
        for lv in (1, 6, 9):
            cases.append(("flushes_l%d" % lv, raw_deflate(fq, lv, flush_at=((13001, zlib.Z_SYNC_FLUSH), (26003, zlib.Z_FULL_FLUSH))), fq))
        cases.append(("flush_then_reference", raw_deflate(b"0123456789abcdefghij" * 2, 6, flush_at=((20, zlib.Z_SYNC_FLUSH),)), b"0123456789abcdefghij" * 2))
        zlib_cases.made = cases
    return zlib_cases.made


def writer_cases():
    """-> [(name, deflate bytes)]: the valid streams only the writer makes"""
    rng = random.Random(5)
    out = []
    w = DW.BitWriter()                                              # a match at distance 32768 and length 258, then one at distance 1
    DW.fixed(w, list(rng.randbytes(32768)) + [(258, 32768), (258, 1), (3, 32768)], True)
    out.append(("distance_32768_length_258", w.done()))
    # codes of 1..15 bits in both alphabets: the symbols used most below have the 15-bit codes
    ll = [0] * 286
    for l, s in zip(list(range(1, 15)) + [15, 15], (65, 67, 71, 84, 78, 10, 257, 258, 259, 260, 285, 284, 66, 68, 256, 69)):
        ll[s] = l
    d = [0] * 16
    for l, s in zip(list(range(1, 15)) + [15, 15], range(15, -1, -1)):
        d[s] = l
    w = DW.BitWriter()
    DW.dynamic(w, [69, 68, 66, 65, 69, 69, (3, 1), (258, 2), ("len284", 1), (4, 3), 10, 78, (6, 200)], True, ll, d)
    out.append(("codes_of_15_bits", w.done()))
    w = DW.BitWriter()                                              # a single distance code: the one incomplete set that is legal
    ll = [0] * 265
    ll[97], ll[98], ll[256], ll[257 + 7] = 1, 2, 3, 3
    DW.dynamic(w, [97, 98, (10, 1), 97, (10, 1)], True, ll, [1])
    out.append(("single_distance_code", w.done()))
    # repeat codes across the border between the two alphabets' lengths
    w = DW.BitWriter()                                              # 16: ... 4 5 5 | 5 5 5 5 3 2 1
    ll = [0] * 259
    ll[97], ll[98], ll[99], ll[256], ll[257], ll[258] = 1, 2, 3, 4, 5, 5
    ops = DW.dynamic(w, [97, 98, 99, (3, 1), (4, 2), (3, 5), (4, 7)], True, ll, [5, 5, 5, 5, 3, 2, 1])
    assert any(o[0] == 16 and o[2] < 259 < o[2] + o[3] for o in ops)
    out.append(("repeat_16_across_the_border", w.done()))
    w = DW.BitWriter()                                              # 17: ... 3 3 0 0 | 0 0 0 1 2 3 3
    ll = [0] * 260
    ll[97], ll[98], ll[256], ll[257] = 1, 2, 3, 3
    ops = DW.dynamic(w, [97] * 6 + [98] * 6 + [(3, 9), 97, (3, 4)], True, ll, [0, 0, 0, 1, 2, 3, 3])
    assert any(o[0] == 17 and o[2] < 260 < o[2] + o[3] for o in ops)
    out.append(("repeat_17_across_the_border", w.done()))
    w = DW.BitWriter()                                              # 18, with HLIT 286 and HDIST 30: 28 zeros | 26 zeros 1 2 3 3
    ll = [0] * 286
    ll[97], ll[98], ll[256], ll[257] = 1, 2, 3, 3
    ops = DW.dynamic(w, [97] * 5000 + [98] * 3200 + [(3, 8193), 97, (3, 8200)], True, ll, [0] * 26 + [1, 2, 3, 3])
    assert any(o[0] == 18 and o[2] < 286 < o[2] + o[3] for o in ops)
    out.append(("repeat_18_across_the_border_286_and_30_codes", w.done()))
    w = DW.BitWriter()                                              # length symbol 284 with extra 31: another spelling of 258
    DW.fixed(w, [120, 121, ("len284", 2), ("len284", 1), (258, 260)], True)
    out.append(("symbol_284_extra_31", w.done()))
    w = DW.BitWriter()                                              # the final block is stored and empty
    DW.fixed(w, list(b"not the last block") + [(5, 4)], False)
    DW.stored(w, b"", False)
    DW.stored(w, b"stored in the middle", False)
    DW.stored(w, b"", True)
    out.append(("final_block_stored_and_empty", w.done()))
    return out


def corrupt_cases():
    """-> [(name, deflate bytes, isize, status class)]"""
    good = raw_deflate(b"ACGTTGCA" * 40 + b"the end", 6)
    n = 8 * 40 + 7
    out = []
    w = DW.BitWriter()
    w.bits(1, 1); w.bits(3, 2); w.bits(0, 13)
    out.append(("block_type_3", w.done(), 5, INVALID))
    w = DW.BitWriter()
    DW.stored(w, b"hello", True, nlen=5 ^ 0xfffe)
    out.append(("nlen_wrong", w.done(), 5, INVALID))
    w = DW.BitWriter()
    ll = [0] * 257
    ll[97], ll[98], ll[256] = 1, 1, 1
    DW.dynamic(w, [97, 98], True, ll, [1])
    out.append(("over_subscribed", w.done(), 2, INVALID))
    w = DW.BitWriter()
    DW.fixed(w, [97, (3, 2)], True)
    out.append(("distance_before_the_start", w.done(), 4, INVALID))
    out.append(("input_cut_short", good[:len(good) - 3], n, INVALID))
    out.append(("isize_plus_1_bytes", good, n - 1, LENGTH))
    out.append(("isize_minus_1_bytes", good, n + 1, LENGTH))
    return out


def zlib_says(comp, isize):
    """what the host path makes of a block: None fine, "invalid" (Z_DATA_ERROR) or "length" """
    z = zlib.decompressobj(-15)
    try:
        got = z.decompress(comp, isize + 1)
    except zlib.error:
        return "invalid"
    return None if z.eof and len(got) == isize else "length"


# ---- the writer against zlib (no GPU, no emulator) ----
def test_writer_streams_are_what_zlib_reads():
    for name, comp in writer_cases():
        data = zlib.decompress(comp, -15)
        assert len(data) > 0 and len(comp) <= MEMBER_MAX and len(data) <= 65536, name
    by = dict(writer_cases())
    assert len(zlib.decompress(by["distance_32768_length_258"], -15)) == 32768 + 258 + 258 + 3
    assert zlib.decompress(by["single_distance_code"], -15) == DW.expand([97, 98, (10, 1), 97, (10, 1)])
    assert zlib.decompress(by["symbol_284_extra_31"], -15) == DW.expand([120, 121, (258, 2), (258, 1), (258, 260)])
    assert zlib.decompress(by["final_block_stored_and_empty"], -15) == DW.expand(list(b"not the last block") + [(5, 4)]) + b"stored in the middle"
    for name, comp, isize, cls in corrupt_cases():
        said = zlib_says(comp, isize)
        if name == "input_cut_short":                               # (zlib waits for more input: the host path reports the length)
            assert said == "length", name
        else:
            assert said == ("invalid" if cls is INVALID else "length"), (name, said)
    # the claims of the module's docstring about zlib (1.2.11 and later)
    rnd = random.Random(1).randbytes(65536)
    assert len(raw_deflate(rnd[:65280], 0)) == 65290 <= MEMBER_MAX < len(raw_deflate(rnd, 0)) == 65546
    for st in STRATEGIES:
        assert zlib.decompress(raw_deflate(rnd[:300], 6, st), -15) == rnd[:300]
    kinds = {"acgt", "fastq", "one_byte", "random", "period_2", "period_3", "period_5", "period_67"}
    assert kinds == set(payloads(10, 1))
    for n in SIZES:                                                 # every size with every pair, every kind at every size
        mine = [c[0] for c in zlib_cases() if ("_%d_l" % n) in c[0]]
        assert {m.rsplit("_%d_" % n, 1)[1] for m in mine} == {"l%d_s%d" % p for p in PAIRS} or n >= 65535, n
        assert {m.rsplit("_%d_" % n, 1)[0] for m in mine} >= kinds - ({"random", "acgt"} if n > 65280 else set()), n
    big = [c for c in zlib_cases() if len(c[2]) == 65536]
    assert len(big) >= 12 and all("random" not in c[0] for c in big)


def run_blocks(lib, blocks, gap_seed=3):
    """blocks: [(deflate bytes, isize)] in one launch: input offsets at every residue mod 4, output offsets at every residue mod 16,
    GUARD bytes between the ranges -> (the ranges' bytes, status, True if every guard byte is untouched)"""
    rng = random.Random(gap_seed)
    comp, in_off, in_len, out_off, isize, o = bytearray(), [], [], [], [], 0
    for i, (c, n) in enumerate(blocks):
        comp += rng.randbytes(1 + i % 7)
        o += 1 + (i * 5 + i // 16) % 16
        in_off.append(len(comp)); in_len.append(len(c)); out_off.append(o); isize.append(n)
        comp += c
        o += n
    out = np.full(o + 9, GUARD, np.uint8)
    got, status = chunkpass.inflate_blocks(bytes(comp), in_off, in_len, out_off, isize, out=out, lib=lib)
    mask = np.ones(out.shape[0], bool)
    for a, n in zip(out_off, isize):
        mask[a:a + n] = False
    return [got[a:a + n].tobytes() for a, n in zip(out_off, isize)], status.tolist(), bool((got[mask] == GUARD).all()), (in_off, out_off)


# ---- 1. byte-exact ----
def check_exact(lib):
    cases = [(name, comp, data) for name, comp, data in zlib_cases()] + [(name, comp, zlib.decompress(comp, -15)) for name, comp in writer_cases()]
    assert len(cases) > 700
    rng = random.Random(9)
    rng.shuffle(cases)                                              # (large and small members next to each other)
    got, status, guards, (in_off, out_off) = run_blocks(lib, [(c, len(d)) for _, c, d in cases])
    assert {a % 4 for a in in_off} == set(range(4)) and {a % 16 for a in out_off} == set(range(16))
    bad = [name for (name, _, d), g, st in zip(cases, got, status) if st != 0 or g != d]
    assert not bad, "%d of %d blocks differ from zlib's bytes or have a status: %s" % (len(bad), len(cases), bad[:10])
    assert guards


# ---- 2. corrupt streams ----
def check_corrupt(lib):
    good = [(raw_deflate(p, 6), p) for p in (b"left neighbour " * 30, random.Random(2).randbytes(700), b"right neighbour" * 500)]
    for name, comp, n, cls in corrupt_cases():
        blocks = [(good[0][0], len(good[0][1])), (good[1][0], len(good[1][1])), (comp, n), (good[2][0], len(good[2][1]))]
        got, status, guards, _ = run_blocks(lib, blocks)
        print(name, status)
        assert status[2] in cls and status[2] != 0, (name, status)
        assert status[:2] == [0, 0] and status[3] == 0 and got[0] == good[0][1] and got[1] == good[1][1] and got[3] == good[2][1], name
        assert guards, name
    assert set(INVALID).isdisjoint(LENGTH)


def test_emulated_inflate_is_byte_exact(emu_lib):
    check_exact(emu_lib)


def test_emulated_inflate_corrupt_streams(emu_lib):
    check_corrupt(emu_lib)


@pytest.mark.gpu
def test_gpu_inflate_is_byte_exact(gpu_lib):
    check_exact(gpu_lib)


@pytest.mark.gpu
def test_gpu_inflate_corrupt_streams(gpu_lib):
    check_corrupt(gpu_lib)

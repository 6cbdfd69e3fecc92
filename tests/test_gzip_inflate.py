"""A plain gzip stream inflated by speculative spans (longqc_amd/csrc/kernels_gzip.hpp, gzip.hpp) through the array call
lqinflate_gzip / chunkpass.inflate_gzip, under the wave emulator and on the GPU.  The inputs are zlib.compressobj's, the truth is
zlib.decompress of the same bytes; about 300 KB of FASTQ text and spans of 1024 to 8192 compressed bytes, so that a file has many
spans and a case takes seconds.  Every case returns the text byte for byte:
  1. levels 1, 6 and 9 at memLevel 8; memLevel 1 (a block every few hundred bytes: many boundaries per span); memLevel 9 at 1024-byte
     spans (most spans hold no boundary);
  2. Z_FIXED and level 0: the search finds nothing there, every launch is its first span alone;
  3. Z_SYNC_FLUSH and Z_FULL_FLUSH every 10 KB (pigz's shape: empty stored blocks between the others);
  4. three members, one of them empty, one with FNAME, FEXTRA and FHCRC;
  5. repeats exactly 32 768 and 32 767 bytes apart: matches at the greatest distance, across span borders;
  6. a 4 MiB run of one byte: the block fits no span's region, not after the doubling either, and zlib makes it;
  7. outputs whose length is no multiple of 16 landing at every residue mod 16 of the destination;
  8. what `stats` must say, so that no case passes through zlib alone."""
import random
import struct
import zlib

import pytest

from longqc_amd import api, chunkpass
from tests import test_filechunks as TF

_TEXT = {}


def fastq_text():
    """about 300 KB of multi-line FASTQ: test_filechunks' records, seven seeds"""
    if "t" not in _TEXT:
        _TEXT["t"] = b"".join(TF.fastq_bytes(TF.rand_records(seed, b"ACGT"), 60) for seed in range(40, 47))
        assert 250000 < len(_TEXT["t"]) < 400000 and len(_TEXT["t"]) % 16
    return _TEXT["t"]


def gz(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = []
    for k, i in enumerate(range(0, len(data), flush_every)):
        out.append(c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH if k % 3 == 2 else zlib.Z_SYNC_FLUSH))
    return b"".join(out) + c.flush()


def member(data, name=None, extra=None, hcrc=False, level=6):
    """one gzip member with the optional header fields of RFC 1952"""
    flg = (8 if name is not None else 0) | (4 if extra is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return h + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def inflate(lib, comp, span):
    got, st = chunkpass.inflate_gzip(comp, span, lib=lib)
    print(span, len(comp), st)
    assert st["bytes_device"] + st["bytes_zlib"] == len(got)
    return got, st


def check_levels(lib):
    text = fastq_text()
    for level, mem, span in ((1, 8, 8192), (6, 8, 4096), (9, 8, 2048), (6, 1, 1024), (6, 9, 1024)):
        comp = gz(text, level, mem)
        got, st = inflate(lib, comp, span)
        assert got == text == zlib.decompress(comp, 31), (level, mem, span)
        n_spans = -(-len(comp) // span)
        if mem == 8 and level in (6, 9):                            # 8.
            assert st["spans_accepted"] >= 2 and st["markers_resolved"] > 0 and st["bytes_zlib"] == 0, st
        if mem == 1:                                                # (its small blocks are often fixed-code ones, which nobody looks for)
            assert st["spans_accepted"] >= 2 and st["bytes_zlib"] == 0, st
        if mem == 9:
            assert st["spans_found"] < n_spans // 4, (st, n_spans)


def check_unsearched(lib):
    text = fastq_text()
    for level, strategy in ((6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
        comp = gz(text, level, 8, strategy)
        got, st = inflate(lib, comp, 4096)
        assert got == text, (level, strategy)
        if strategy == zlib.Z_FIXED:
            assert st["spans_found"] == 0 and st["spans_accepted"] == 0, st


def check_flushes(lib):
    text = fastq_text()
    comp = gz(text, 6, 8, flush_every=10000)
    got, st = inflate(lib, comp, 2048)
    assert got == text == zlib.decompress(comp, 31)
    assert st["spans_accepted"] >= 2, st


def check_members(lib):
    text = fastq_text()
    a, b = text[:100001], text[100001:]
    comp = member(a, name=b"reads.fq", extra=b"XY\x03\0abc", hcrc=True) + member(b"") + member(b, level=9)
    got, st = inflate(lib, comp, 2048)
    assert got == a + b
    d = zlib.decompressobj(31)
    assert d.decompress(comp) == a and d.unused_data[:2] == b"\x1f\x8b"      # (zlib reads the first header the same way)
    # a header CRC that is wrong, a method that is not deflate: the stream is refused
    bad = bytearray(comp); bad[10 + 9 + 9] ^= 1                              # the first member's FHCRC: behind ten bytes, FEXTRA and FNAME
    for data in (bytes(bad), member(a) + b"\x1f\x8b\x07" + member(b)[3:]):
        with pytest.raises(api.LqcovError) as e:
            chunkpass.inflate_gzip(data, 2048, lib=lib, out_cap=len(text) + 64)
        assert e.value.code == -2 and "not a complete gzip stream" in str(e.value)


def check_max_distance(lib):
    rng = random.Random(9)
    out = bytearray(rng.choices(b"ACGTN", k=33000))
    for k in range(9):                                              # every part copies a run from exactly 32768 / 32767 back
        dist = 32768 if k % 2 == 0 else 32767
        for _ in range(40):
            run = rng.randrange(3, 259)
            out += out[len(out) - dist:len(out) - dist + run]
            out += bytes(rng.choices(b"ACGTN", k=rng.randrange(1, 600)))
    text = bytes(out)
    comp = gz(text, 9, 4)                                           # (memLevel 4: a block every 1023 symbols, so that spans are found)
    got, st = inflate(lib, comp, 1024)
    assert got == text
    assert st["markers_resolved"] > 0 and st["spans_accepted"] >= 2 and st["bytes_zlib"] == 0, st


def check_long_run(lib):
    text = b"A" * (4 << 20) + b"CGT"
    comp = gz(text, 6, 8)
    got, st = inflate(lib, comp, 1024)
    assert got == text
    assert st["bytes_zlib"] >= 4 << 20 and st["launches"] >= 2, st     # the region, the doubled region, then zlib


def check_residues(lib):
    text = fastq_text()[:30000]
    for r in range(16):
        # the second member's bytes land at residue r; its spans' lengths are whatever the blocks give
        first, second = text[:r], text[r:r + 20011 + r]
        comp = member(first) + gz(second, 6, 1)
        got, st = chunkpass.inflate_gzip(comp, 1024, lib=lib)
        assert got == first + second and len(got) % 16, r
        assert st["spans_accepted"] >= 2, (r, st)


CHECKS = [check_levels, check_unsearched, check_flushes, check_members, check_max_distance, check_long_run, check_residues]


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_emulated_gzip_inflate(emu_lib, check):
    check(emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_gpu_gzip_inflate(gpu_lib, check):
    check(gpu_lib)

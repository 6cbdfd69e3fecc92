"""k_crc32_ranges (kernels_crc32.hpp) through chunkpass.crc32_ranges against zlib.crc32, exact: every length at which a lane's share,
the wave's merge, the bytes behind the last full word or the host's merge of units changes, at every start residue mod 16, over
random bytes, zeros (a wrong start value or merge passes them through unnoticed only if it is right), 0xFF and FASTQ text."""
import random
import zlib

import numpy as np
import pytest

from longqc_amd import api, chunkpass
from tests import test_launch_caps as LC

UNIT = LC.header_define("LQ_CRC_UNIT")
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
           65279, 65280, 65535, 65536, 65537, 200001, 3 * UNIT + 5]
PAD = 16 + 31                                                       # bytes around the ranges


def fastq_text(n, rng):
    out = bytearray()
    i = 0
    while len(out) < n:
        l = rng.randrange(20, 300)
        out += b"@read%d extra\n" % i + bytes(rng.choices(b"ACGT", k=l)) + b"\n+\n" + bytes(rng.choices(b"!#5?I", k=l)) + b"\n"
        i += 1
    return bytes(out[:n])


def contents(n):
    rng = random.Random(7)
    return {"random": rng.randbytes(n), "zeros": bytes(n), "ones": b"\xff" * n, "fastq": fastq_text(n, rng)}


@pytest.fixture(scope="module")
def buffers():
    return contents(max(LENGTHS) + PAD + 16)


def check_lengths(lib, buffers):
    """every length at every residue, all in one call per content"""
    off, length = [], []
    for k, n in enumerate(LENGTHS):
        for res in range(16):
            if n > 70000 and res not in (0, 1, 15):                 # (the long ones: the merge of units, three residues)
                continue
            off.append(16 + res + (k % 3) * 16); length.append(n)
    for what, data in buffers.items():
        want = np.array([zlib.crc32(data[o:o + l]) for o, l in zip(off, length)], np.uint32)
        got = chunkpass.crc32_ranges(data, off, length, lib=lib)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %s" % (what, [(off[i], length[i], hex(got[i]), hex(want[i])) for i in bad[:8]])


def check_many_ranges(lib):
    """touching, overlapping and nested ranges in one call; what lies around them does not matter"""
    rng = random.Random(11)
    data = bytearray(rng.randbytes(6000))
    off, length, at = [], [], 5
    while at < 5000:                                                # touching
        l = min(rng.randrange(0, 90), 5000 - at)
        off.append(at); length.append(l); at += l
    for _ in range(300):                                            # overlapping
        o = rng.randrange(5, 5000)
        off.append(o); length.append(rng.randrange(0, 5000 - o + 1))
    want = np.array([zlib.crc32(bytes(data[o:o + l])) for o, l in zip(off, length)], np.uint32)
    got = chunkpass.crc32_ranges(bytes(data), off, length, lib=lib)
    assert (got == want).all(), np.flatnonzero(got != want)[:10]
    data[:5] = b"\xaa" * 5; data[5000:] = bytes(1000)              # the bytes around the ranges change, the result does not
    again = chunkpass.crc32_ranges(bytes(data), off, length, lib=lib)
    assert (again == want).all(), np.flatnonzero(again != want)[:10]


def check_arguments(lib):
    data = bytes(range(100))
    assert chunkpass.crc32_ranges(data, [], [], lib=lib).shape == (0,)
    assert chunkpass.crc32_ranges(data, [100, 0], [0, 100], lib=lib).tolist() == [0, zlib.crc32(data)]
    assert chunkpass.crc32_ranges(b"", [0], [0], lib=lib).tolist() == [0]
    for off, length in (([101], [0]), ([100], [1]), ([0], [101]), ([50, 2 ** 63], [1, 2 ** 63])):
        with pytest.raises(api.LqcovError) as e:
            chunkpass.crc32_ranges(data, off, length, lib=lib)
        assert e.value.code == -1, e.value                          # LQCOV_E_ARG


def test_emulated_crc32_lengths_and_residues(emu_lib, buffers):
    check_lengths(emu_lib, buffers)


def test_emulated_crc32_many_ranges(emu_lib):
    check_many_ranges(emu_lib)


def test_emulated_crc32_arguments(emu_lib):
    check_arguments(emu_lib)


@pytest.mark.gpu
def test_gpu_crc32_lengths_and_residues(gpu_lib, buffers):
    check_lengths(gpu_lib, buffers)


@pytest.mark.gpu
def test_gpu_crc32_many_ranges(gpu_lib):
    check_many_ranges(gpu_lib)


@pytest.mark.gpu
def test_gpu_crc32_arguments(gpu_lib):
    check_arguments(gpu_lib)

"""The .mmi format alone (longqc_amd/csrc/mmi.hpp; mm_idx_dump / mm_idx_load, index.c:390-479), without a handle, a device or
the emulator: the header is compiled with g++ behind tests/emu/mmi_shim.cpp and fed files packed here by hand.  A part of two
sequences and three minimizers -- one singleton, one list of two -- in b = 2 bucket bits (the reader takes any b <= 30, the
writer the b of its header; the engine's files have 14): tens of bytes reach every branch.  What the engine does with such a
part is in test_mmi.py and test_gpu_parity.py."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests.conftest import ROOT
from tests.test_mmi import parse_mmi

MAGIC = b"MMI\x02"
NO_SEQ = 2
TRUNCATED = "truncated index file"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mmi_shim") / "mmi_shim.so")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(ROOT, "tests", "emu", "mmi_shim.cpp"), "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    lib = C.CDLL(so)
    lib.shim_mmi_write.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]
    lib.shim_mmi_read.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    return lib


def pieces(header, seqs, buckets, S=b""):
    """The fields of one part in file order, [(what, bytes)]: header = (w, k, b, n_seq, flag), seqs = [(name, length)],
    buckets = [(n_p, positions, size, [(key, value)])] -- n_p and size are stated, not derived, so that a file may lie."""
    out = [("magic", MAGIC), ("header", struct.pack("<5I", *header))]
    for name, ln in seqs:
        out += [("name length", struct.pack("<B", len(name))), ("name", name), ("sequence length", struct.pack("<I", ln))]
    for n_p, p, size, kv in buckets:
        out += [("n_p", struct.pack("<i", n_p)), ("position array", struct.pack("<%dQ" % len(p), *p)), ("size", struct.pack("<I", size))]
        out += [("key/value pair", struct.pack("<2Q", k, v)) for k, v in kv]
    return out + [("sequences", S)]


def join(ps):
    return b"".join(b for _, b in ps)


# two sequences, 14 bases = two words of 4-bit codes; minimizer 13 = 3 << 2 | 1 at two positions, minimizer 22 = 5 << 2 | 2 at one
W, K, B = 5, 12, 2
SEQS = [(b"s0", 9), (b"s1", 5)]
YA, YB, YC = 0 << 32 | 7 << 1, 1 << 32 | 3 << 1 | 1, 0 << 32 | 4 << 1 | 1
S_WORDS = [0x32103210, 0x00213021]
BUCKETS = [(0, [], 0, []), (2, [YA, YB], 1, [(3 << 1, 0 << 32 | 2)]), (0, [], 1, [(5 << 1 | 1, YC)]), (0, [], 0, [])]
INDEX = dict(hkey=[13, 22], hstart=[0, 2], hcnt=[2, 1], hpos=[YA, YB, YC])
X_Y = [(13 << 8, YA), (13 << 8, YB), (22 << 8, YC)]


def part_bytes(seqs=SEQS, flag=0):
    return join(pieces((W, K, B, len(seqs), flag), seqs, BUCKETS, b"" if flag & NO_SEQ else struct.pack("<2I", *S_WORDS)))


def arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def write_part(shim, path, seqs=SEQS, flag=0, b=B, append=False, index=INDEX):
    err = C.create_string_buffer(256)
    rc = shim.shim_mmi_write(path.encode(), int(append), arr(C.c_uint32, [W, K, b, len(seqs), flag]), b"".join(n for n, _ in seqs), arr(C.c_uint32, [len(n) for n, _ in seqs]),
                             arr(C.c_uint32, [l for _, l in seqs]), len(index["hkey"]), arr(C.c_uint64, index["hkey"]), arr(C.c_uint64, index["hstart"]), arr(C.c_uint32, index["hcnt"]),
                             len(index["hpos"]), arr(C.c_uint64, index["hpos"]), len(S_WORDS), arr(C.c_uint32, S_WORDS), err, 256)
    assert rc == 0, err.value


def read_part(shim, path, offset=0):
    """-> (1, dict(header, seqs, xy, end)) | (0, None) | (-1, message)"""
    off, n_xy, err = C.c_int64(offset), C.c_uint64(0), C.create_string_buffer(256)
    hdr, name_len, lens = (C.c_uint32 * 5)(), (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    names, x, y = C.create_string_buffer(4096), (C.c_uint64 * 64)(), (C.c_uint64 * 64)()
    rc = shim.shim_mmi_read(path.encode(), C.byref(off), hdr, names, 4096, name_len, lens, 8, x, y, 64, C.byref(n_xy), err, 256)
    if rc == 0:
        return 0, None
    if rc < 0:
        return rc, err.value.decode()
    seqs, o = [], 0
    for i in range(hdr[3]):
        seqs.append((names.raw[o:o + name_len[i]], lens[i])); o += name_len[i]
    return 1, dict(header=tuple(hdr), seqs=seqs, xy=[(x[i], y[i]) for i in range(n_xy.value)], end=off.value)


def put(tmp_path, data, name="a.mmi"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.mark.parametrize("flag", [0, 1, NO_SEQ], ids=["with sequences", "-H", "no sequences"])
def test_written_bytes_are_the_hand_packed_ones_and_read_back(shim, tmp_path, flag):
    path = str(tmp_path / "w.mmi")
    write_part(shim, path, flag=flag)
    data = open(path, "rb").read()
    assert data == part_bytes(flag=flag)
    (p,) = parse_mmi(data)
    assert p["header"] == (W, K, B, 2, flag) and p["seqs"] == SEQS
    assert p["index"] == {13: [YA, YB], 22: [YC]}
    assert p["S"] == (b"" if flag & NO_SEQ else struct.pack("<2I", *S_WORDS))
    rc, got = read_part(shim, path)
    assert rc == 1 and got["header"] == p["header"] and got["seqs"] == SEQS
    assert got["xy"] == X_Y and all(x == m << 8 for (x, _), m in zip(got["xy"], [13, 13, 22]))
    assert got["end"] == len(data)                               # the sequences are stepped over, not read


def test_parts_follow_each_other_and_other_bytes_end_them(shim, tmp_path):
    """a file of several parts is the parts end to end (index.c:500-540); the end of the file, or anything but the magic where a
    part would start, is "no part" and no error"""
    path = str(tmp_path / "two.mmi")
    write_part(shim, path)
    write_part(shim, path, seqs=[(b"t", 14)], append=True)
    one = len(part_bytes())
    assert open(path, "rb").read() == part_bytes() + part_bytes(seqs=[(b"t", 14)])
    rc, a = read_part(shim, path)
    assert rc == 1 and a["end"] == one and a["seqs"] == SEQS
    rc, b = read_part(shim, path, a["end"])
    assert rc == 1 and b["seqs"] == [(b"t", 14)] and b["xy"] == X_Y
    assert read_part(shim, path, b["end"]) == (0, None)          # the end of the file
    assert read_part(shim, put(tmp_path, b"")) == (0, None)      # zero bytes
    assert read_part(shim, put(tmp_path, b"MMI\x01")) == (0, None)   # four bytes of another magic
    assert read_part(shim, put(tmp_path, b"MM")) == (0, None)    # not even four
    tail = put(tmp_path, part_bytes() + b">seq", "tail.mmi")
    assert read_part(shim, tail)[0] == 1 and read_part(shim, tail, one) == (0, None)


def test_names_of_255_bytes_and_names_cut_at_a_nul(shim, tmp_path):
    long_name = bytes(range(1, 256))
    path = str(tmp_path / "n.mmi")
    write_part(shim, path, seqs=[(long_name, 9), (b"s1", 5)])
    data = open(path, "rb").read()
    assert data == part_bytes(seqs=[(long_name, 9), (b"s1", 5)])
    assert parse_mmi(data)[0]["seqs"] == [(long_name, 9), (b"s1", 5)]
    rc, got = read_part(shim, path)
    assert rc == 1 and got["seqs"] == [(long_name, 9), (b"s1", 5)] and got["xy"] == X_Y
    # the reference holds a name as a C string (index.c:448-450): what follows a NUL is dropped, the file's length byte still counts
    rc, got = read_part(shim, put(tmp_path, part_bytes(seqs=[(b"ab\0cd", 9), (b"\0x", 5)])))
    assert rc == 1 and got["seqs"] == [(b"ab", 9), (b"", 5)] and got["xy"] == X_Y


def _cuts():
    """every field of the part after the magic, cut in its middle (a one-byte field: the file ends right before it)"""
    ps = pieces((W, K, B, 2, 0), SEQS, BUCKETS, struct.pack("<2I", *S_WORDS))
    cuts, at = [], 0
    for i, (what, b) in enumerate(ps):
        if what not in ("magic", "sequences") and b:
            cuts.append(pytest.param(at + len(b) // 2, id="%s (field %d)" % (what, i)))
        at += len(b)
    return cuts


@pytest.mark.parametrize("cut", _cuts())
def test_a_file_that_ends_inside_a_part_is_truncated(shim, tmp_path, cut):
    assert read_part(shim, put(tmp_path, part_bytes()[:cut])) == (-1, TRUNCATED)


def test_every_field_kind_is_among_the_cuts():
    kinds = {p.id.split(" (")[0] for p in _cuts()}
    assert kinds == {"header", "name length", "name", "sequence length", "n_p", "position array", "size", "key/value pair"}


def test_refusals_of_a_corrupt_part(shim, tmp_path):
    def refused(header, buckets):
        return read_part(shim, put(tmp_path, join(pieces(header, SEQS, buckets, struct.pack("<2I", *S_WORDS)))))
    assert refused((W, K, B, 2, 0), [(-1, [], 0, [])] + BUCKETS[1:]) == (-1, TRUNCATED)                 # n_p = -1
    assert read_part(shim, put(tmp_path, MAGIC + struct.pack("<5I", W, K, 31, 0, 0))) == (-1, "corrupt index file (bucket bits)")
    assert refused((W, K, 31, 2, 0), BUCKETS) == (-1, "corrupt index file (bucket bits)")
    assert read_part(shim, put(tmp_path, join(pieces((W, K, 30, 0, 0), [], BUCKETS[:1])))) == (-1, TRUNCATED)   # b = 30 is taken: the buckets run out
    for start, n in [(0, 3), (1, 2), (2, 1), (0xffffffff, 2)]:                                           # start + n > n_p = 2
        assert refused((W, K, B, 2, 0), [BUCKETS[0], (2, [YA, YB], 1, [(3 << 1, start << 32 | n)])] + BUCKETS[2:]) == (-1, "corrupt index file (position list)")
    rc, got = refused((W, K, B, 2, 0), [BUCKETS[0], (2, [YA, YB], 1, [(3 << 1, 1 << 32 | 1)])] + BUCKETS[2:])   # start + n == n_p holds
    assert rc == 1 and got["xy"] == [(13 << 8, YB), (22 << 8, YC)]

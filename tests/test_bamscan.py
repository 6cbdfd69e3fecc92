"""The record walk of an unaligned BAM on the device (chunkpass.scan_bam_records over lqbam_scan: k_bam_candidates, k_bam_link, k_fx_jump,
k_bam_emit, kernels_bamscan.hpp) against the domain of DESIGN 8 (15) as `model` states it in Python, under the wave emulator and on the
GPU.  The comparison is exact: rows, both segment lists, the counts and the resume position.  The inputs are written by
tests/bam_writer.py; the decoys -- bytes that are no record of the chain but pass the cheap part of the test -- are shown in Python to
be candidates before the scan sees them."""
import ctypes as C
import struct

import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import bam_writer as BW
from tests import test_launch_caps as LC

FF8 = b"\xff" * 8
HDR = len(BW.header())


def fields(data, o):
    block_size, = struct.unpack_from("<I", data, o)
    l_seq, = struct.unpack_from("<I", data, o + 20)
    return block_size, data[o + 12], data[o + 16] | data[o + 17] << 8, l_seq


def vouched(data, o):
    """the domain: is offset o of data a record the device vouches for"""
    n = len(data)
    if o + 36 > n or data[o + 4:o + 12] != FF8 or data[o + 24:o + 32] != FF8:
        return False
    block_size, l_name, n_cigar, l_seq = fields(data, o)
    if l_name < 1 or l_seq > 2 ** 31 - 1 or block_size > 2 ** 31 - 1:
        return False
    if block_size < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq or o + 4 + block_size > n:
        return False
    return data[o + 36 + l_name - 1] == 0


def cheap(data, o):
    """the cheap part of the test, what makes an offset a candidate"""
    return o + 36 <= len(data) and data[o + 4:o + 12] == FF8 and data[o + 24:o + 32] == FF8 and data[o + 23] < 0x80


def model(data, start, with_qual):
    rows, sseg, qseg, o, d = [], [], [], start, 0
    while vouched(data, o):
        block_size, l_name, n_cigar, l_seq = fields(data, o)
        rows.append([o + 36, data.index(0, o + 36) - (o + 36), l_seq, int(with_qual)])
        src = o + 36 + l_name + 4 * n_cigar
        if l_seq:
            sseg.append([src, d])
            qseg.append([src + (l_seq + 1) // 2 if with_qual else chunkpass.GATHER_FILL, d])
        d += l_seq
        o += 4 + block_size
    return rows, sseg, qseg, o                                      # (the first chain element that is not vouched; at most len(data))


def check_scan(lib, data, start=HDR, want_rows=None, want_resume=None):
    """both quality modes against the model -> the rows"""
    for with_qual in (False, True):
        rows, sseg, qseg, resume = chunkpass.scan_bam_records(data, start, with_qual, lib=lib)
        m_rows, m_sseg, m_qseg, m_resume = model(data, start, with_qual)
        assert rows.tolist() == m_rows, (len(rows), len(m_rows), start)
        assert sseg.tolist() == m_sseg and qseg.tolist() == m_qseg, start
        assert resume == m_resume, (resume, m_resume, start)
    if want_rows is not None:
        assert len(m_rows) == want_rows, (len(m_rows), want_rows)
    if want_resume is not None:
        assert m_resume == want_resume, (m_resume, want_resume)
    return rows


def offsets(recs, at=HDR):
    """where each record starts, and the end of the last"""
    out = [at]
    for r in recs:
        out.append(out[-1] + len(r))
    return out


def seq(rng, l):
    return bytes(rng.choice(np.frombuffer(BW.CODES, np.uint8), l))


def some_records(seed, n=12):
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(10, 90)) for _ in range(n)]
    return [BW.record(b"read%d" % i, seq(rng, l), bytes(rng.integers(0, 94, l).astype(np.uint8)) if i % 3 else None) for i, l in enumerate(lens)]


def check_boundaries(lib):
    recs = some_records(1)
    data = BW.header() + b"".join(recs)
    at = offsets(recs)
    check_scan(lib, data, want_rows=len(recs), want_resume=len(data))          # the last record ends exactly at n
    check_scan(lib, data[:-1], want_rows=len(recs) - 1, want_resume=at[-2])      # one byte short
    check_scan(lib, data[:at[3] + 35], want_rows=3, want_resume=at[3])          # the 36 bytes are not all there
    check_scan(lib, data[:at[3] + 36], want_rows=3, want_resume=at[3])
    check_scan(lib, data, start=len(data), want_rows=0, want_resume=len(data))
    check_scan(lib, b"", start=0, want_rows=0, want_resume=0)
    check_scan(lib, data[:HDR + 10], want_rows=0, want_resume=HDR)


def check_edge_records(lib):
    rng = np.random.default_rng(5)
    recs = []
    for l in (0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 127, 129, 0, 0, 7):
        q = bytes(rng.integers(0, 94, l).astype(np.uint8))
        recs.append(BW.record(b"n%d" % l, seq(rng, l), q))
    recs.append(BW.record(b"", b"ACGTN", bytes(5)))                             # l_read_name 1: the NUL alone
    recs.append(BW.record(b"in\0ner", b"ACG", bytes(3)))                        # strlen stops at the inner NUL
    recs.append(BW.record(b"cig", b"ACGTACGTA", None, cigar=(9 << 4, 77, 0xffffffff)))
    recs.append(BW.record(b"tags", b"TTGCA", bytes(5), tags=b"ipBC" + struct.pack("<I", 40) + bytes(range(40))))
    recs.append(BW.record(b"both", b"T", b"\x11", cigar=(16,), tags=b"XYZ\xff\xff\xff"))
    recs.append(BW.record(b"caf\xc3\xa9", b"AC", bytes(2)))                     # a name byte of 0x80 or more does not end the vouching
    recs.append(BW.record(b"last", b"", None))
    data = BW.header() + b"".join(recs)
    rows = check_scan(lib, data, want_rows=len(recs), want_resume=len(data))
    assert rows[15].tolist()[1:3] == [0, 5] and rows[16].tolist()[1:3] == [2, 3] and rows[20].tolist()[1] == 5
    blob, name_off, first_bad = chunkpass.gather_names(data, rows, lib=lib)      # the rows are lqfx_names'
    assert blob.split(b"\0")[:len(recs)] == [data[a:a + l] for a, l in rows[:, :2].tolist()] and first_bad == 20


def check_decoys(lib):
    rng = np.random.default_rng(9)
    inner = BW.record(b"inner", b"ACGTAC", bytes(6))
    ff_read = BW.record(b"noqual", seq(rng, 70), None)                           # 70 quality bytes of 0xff
    recs = [BW.record(b"a", b"ACGT", bytes(4)),
            BW.record(b"tail", b"GG", bytes(2), tags=b"zzZ" + inner),            # a whole record whose next is the true next record
            BW.record(b"mid", b"CC", bytes(2), tags=b"zzZ" + inner + b"pad:0123"),      # ... whose next lies inside the tags
            ff_read,
            BW.record(b"b", b"ACGTT", bytes(5)),
            BW.record(b"nn", b"N" * 80, None),                                    # 0xff packed bases and 0xff qualities, back to back
            BW.record(b"c", b"A", bytes(1))]
    data = BW.header() + b"".join(recs)
    at = offsets(recs)
    d_tail, d_mid = at[2] - len(inner), at[3] - len(inner) - 8
    assert data[d_tail:d_tail + len(inner)] == inner and data[d_mid:d_mid + len(inner)] == inner
    for o in (d_tail, d_mid):                                                   # they pass even the full test
        assert cheap(data, o) and vouched(data, o) and o not in at
    assert d_tail + len(inner) == at[2] and d_mid + len(inner) not in at
    # the 0xff qualities make offsets in front of the next record candidates (its refID and pos stand where next_refID and next_pos would)
    for k in (3, 5):
        lo, hi = at[k + 1] - 70, at[k + 1]
        assert data[lo:hi] == b"\xff" * 70
        found = [o for o in range(lo - 36, hi) if cheap(data, o)]
        assert found and all(o not in at and not vouched(data, o) for o in found), (k, found)
    check_scan(lib, data, want_rows=len(recs), want_resume=len(data))
    # a decoy as the start is a start like any other: the model follows it as the device does
    check_scan(lib, data, start=d_tail, want_rows=6)
    check_scan(lib, data, start=d_mid, want_rows=1, want_resume=d_mid + len(inner))


def check_stops(lib):
    recs = some_records(3, 7)
    at = offsets(recs)
    good = BW.header() + b"".join(recs)
    o = at[3]
    l_name = good[o + 12]

    def patched(off, new):
        b = bytearray(good)
        b[o + off:o + off + len(new)] = new
        return bytes(b)

    cases = {"refID = 0": patched(4, struct.pack("<i", 0)),
             "block_size too small": patched(0, struct.pack("<i", 40)),
             "l_read_name = 0": patched(12, b"\0"),
             "no NUL": patched(36 + l_name - 1, b"x"),
             "l_seq = 2^31": patched(20, struct.pack("<I", 1 << 31)),
             "pos = 5": patched(8, struct.pack("<i", 5)),
             "next_pos = 0": patched(28, struct.pack("<i", 0)),
             "block_size past the end": patched(0, struct.pack("<i", len(good)))}
    for what, data in cases.items():
        assert not vouched(data, o) and all(vouched(data, a) for a in at[:3]), what
        rows = check_scan(lib, data, want_rows=3, want_resume=o)
        assert len(rows) == 3, what                                             # the records behind it are not reported
        check_scan(lib, data, start=at[4], want_rows=3, want_resume=len(data))  # (they are there)


def check_starts(lib):
    rng = np.random.default_rng(31)
    recs = [BW.record(b"r%d" % i, seq(rng, int(rng.integers(0, 400))), None,
                      tags=bytes(rng.integers(0, 256, int(rng.integers(0, 60))).astype(np.uint8))) for i in range(20)]
    data = BW.header() + b"".join(recs)
    at = offsets(recs)
    for k, a in enumerate(at):
        check_scan(lib, data, start=a, want_rows=20 - k, want_resume=len(data))
    check_scan(lib, data, start=at[1] + 1)                                      # not a boundary: whatever the model says


def check_tile_edges(lib):
    ltile = LC.header_define("LQ_FXSCAN_LINE_TILE")
    assert ltile == 256
    rng = np.random.default_rng(12)
    for n in (255, 256, 257, 600):
        recs = [BW.record(b"t%d" % i, seq(rng, i % 4), None) for i in range(n)]
        data = BW.header() + b"".join(recs)
        check_scan(lib, data, want_rows=n, want_resume=len(data))
        check_scan(lib, data[:-1], want_rows=n - 1)


def check_arguments(lib):
    L = chunkpass._lib(lib)
    data = BW.header() + b"".join(some_records(2, 5))
    buf = np.frombuffer(data, np.uint8)
    rows, ss, qs = np.zeros((8, 4), np.uint32), np.zeros((8, 2), np.uint64), np.zeros((8, 2), np.uint64)
    c = [C.c_uint64() for _ in range(4)]
    refs = [C.byref(x) for x in c]

    def call(bytes_=buf.ctypes.data, n=len(data), start=HDR, rows_=rows.ctypes.data, cap=8, ss_=ss.ctypes.data, qs_=qs.ctypes.data, scap=8, outs=refs):
        return L.lqbam_scan(0, bytes_, n, start, 0, rows_, cap, ss_, qs_, scap, *outs)

    assert call() == 0 and c[0].value == 5 and c[3].value == len(data)
    assert call(start=len(data) + 1) == -1 and b"no parser state" in L.lqreader_last_error(None)
    assert call(bytes_=None) == -1 and b"null buffers" in L.lqreader_last_error(None)
    for k in range(4):
        assert call(outs=[None if i == k else r for i, r in enumerate(refs)]) == -1
    assert call(cap=4) == -1 and b"smaller" in L.lqreader_last_error(None)
    assert call(scap=2) == -1 and call(rows_=None) == -1 and call(ss_=None) == -1 and call(qs_=None) == -1
    assert call(start=len(data)) == 0 and c[0].value == 0 and c[3].value == len(data)
    assert call(bytes_=None, n=0, start=0) == 0 and c[0].value == 0 and c[3].value == 0


CHECKS = [check_boundaries, check_edge_records, check_decoys, check_stops, check_starts, check_tile_edges, check_arguments]


@pytest.mark.parametrize("order", LC.ORDERS)
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_emulated_bam_scan(emu_lib, monkeypatch, check, order):
    LC.set_order(monkeypatch, order)
    check(emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_gpu_bam_scan(gpu_lib, check):
    check(gpu_lib)

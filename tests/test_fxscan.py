"""The record scan of the reader's device mode (chunkpass.scan_records over lqfx_scan: k_fx_lines, k_fx_candidates, k_fx_jump, k_fx_emit,
kernels_fxscan.hpp) against kseq as tests/test_filechunks.py::kseq_records restates it, under the wave emulator and on the GPU.

What is checked for every input and start state: the rows are the first k records kseq reads from that state (name bytes, lengths,
whether there is a quality string); the two segment lists are kseq's own (src, dst) pairs of those records, in destination order, and
the bytes they name are the records' sequences and quality strings; kseq started at the resume state reads the remaining records.
k itself -- how many records the device vouches for -- is written next to every hand-made case, derived from the domain of DESIGN 8 (13):
the header character is a line's first byte; no sequence or quality line is exactly "\\r" and no empty line follows a line that ends
in "\\r\\r"; the record is complete inside the range whatever follows (FASTQ: a quality line that has its line break brings the quality
string to exactly the sequence's length; no '+': the first byte of the next header line is inside the range)."""
import numpy as np
import pytest

from longqc_amd import chunkpass
from tests import test_filechunks as TF
from tests import test_launch_caps as LC


def from_state(data, pos, lc):
    """kseq's records from the parser state (pos, last_char), and the offset its positions count from"""
    base = pos - (1 if lc else 0)
    if lc:
        assert data[base] == lc
    return TF.kseq_records(data[base:]), base


def check_scan(lib, data, want=None, pos=0, lc=0):
    """-> the number of vouched records"""
    rows, sseg, qseg, (rpos, rlc) = chunkpass.scan_records(data, pos, lc, lib=lib)
    (records, src, dst), base = from_state(data, pos, lc)
    k = rows.shape[0]
    assert k <= len(records), (data[:60], k, len(records))
    if want is not None:
        assert k == want, "%r from (%d, %d): the device vouches for %d records, the domain says %d (kseq reads %d)" % (data[:80], pos, lc, k, want, len(records))
    # the rows
    for row, (name, seq, qual) in zip(rows.tolist(), records):
        at, nlen, slen, flags = row
        assert data[at:at + nlen] == name and slen == len(seq) and flags == (1 if qual is not None else 0), (row, name)
        assert data[at - 1] in b"@>" and (at - 1 == 0 or data[at - 2] == 10)
    # the segments: kseq's pairs of the first k records
    total = sum(len(r[1]) for r in records[:k])
    want_pairs = sorted((s + base, d) for s, d in zip(src, dst) if d < total)
    got_pairs = sorted([tuple(x) for x in sseg.tolist()] + [tuple(x) for x in qseg.tolist() if x[0] != chunkpass.GATHER_FILL])
    assert got_pairs == want_pairs
    arr = np.frombuffer(data, dtype=np.uint8)
    for segs, col in ((sseg, 1), (qseg, 2)):
        d = segs[:, 1].astype(np.int64)
        assert (np.diff(d) > 0).all() and (segs.shape[0] == 0 or d[0] == 0) and (total == 0) == (segs.shape[0] == 0)
        ends = np.append(d[1:], total)
        got = b"".join(b"!" * int(e - a) if int(s) == chunkpass.GATHER_FILL else arr[int(s):int(s) + int(e - a)].tobytes()
                       for s, a, e in zip(segs[:, 0].tolist(), d.tolist(), ends.tolist()))
        assert got == b"".join(r[col] if r[col] is not None else b"!" * len(r[1]) for r in records[:k])
    # the resume state
    if k == 0:
        assert (rpos, rlc) == (pos, lc)
    (rest, _, _), _ = from_state(data, rpos, rlc)
    assert rest == records[k:], (data[:60], rpos, rlc)
    return k


# (bytes, records the device vouches for)
HAND = [
    (b"", 0),
    (b"no header\nhere\n\n", 0),                                                    # junk only
    (b"@a\nAC\n+\nII\n\n\n@b\nG\n+\nI\n", 2),                                       # blank lines between records
    (b"xx@r\nAC\n+\nII\n", 0),                                                     # a header in the middle of a line: the host's
    (b"@a\nAC\n+\nII\nxx@r\nAC\n+\nII\n", 1),                                       # ... the device stops in front of it
    (b"@a\nAC\n+\n@I\n@b\nG\n+\nI\n", 2),                                           # a quality line that starts with '@'
    (b"@a\nACGT\n+\nII\n>I\n@b\nG\n+\nI\n", 2),                                     # a second quality line that starts with '>'
    (b"@a\nACGT\n+\nII\n+I\n@b\nG\n+\nI\n", 2),                                     # ... with '+'
    (b"@a\nAC\nGT\nAC\n+\nIIIIII\n@b\nG\n+\nI\n", 2),                               # three sequence lines, one quality line
    (b"@a\nACGTAC\n+\nII\nII\nII\n@b\nG\n+\nI\n", 2),                               # and the reverse
    (b"@r\n+\n\n", 1),                                                             # an empty read takes one quality line
    (b"@r\n\n+\n\n", 1),
    (b"@r\n+\n\n@s\n+\n\n", 2),
    (b"@\nAC\n+\n!!\n", 1),                                                        # an empty name
    (b"@n1\tc d\nAC\n+\nII\n", 1),                                                  # a name ended by a tab
    (b"@n1\r\nAC\r\n+\r\nII\r\n", 1),                                               # ... by '\r'
    (b"@r1\nAC\n+r1\nII\n@r2 x\nG\n+r2 x\nI\n", 2),                                 # the name repeated behind '+'
    (b">a\nAC\nGT\n@b\nAC\n+\nII\n>c\nA\n>d\nC\n", 3),                              # FASTA, FASTQ, FASTA; the last record has no header behind it
    (b"@a\r\nACG\r\n+\r\nIII\r\n>b\r\nAC\r\nGT\r\n>c\r\nA\r\n", 2),                  # CRLF throughout; the last is the host's
    (b"@a\nAC\n+\nII\n@b\nAC\n\r\nGT\n+\nIIII\n@c\nA\n+\nI\n", 1),                  # a lone '\r' line in a sequence
    (b"@a\nAC\n+\nII\n@b\nACGT\n+\nII\n\r\nII\n@c\nA\n+\nI\n", 1),                  # ... in a quality string
    (b"@a\nAC\r\r\n+\nII\r\r\n@b\nG\n+\nI\n", 2),                                   # "\r\r": one '\r' stays
    (b"@a\nAC\n+\nII\n@b\nAC\r\r\nG\n+\nI\r\r\n\nI\n@c\nA\n+\nI\n", 1),             # an empty line behind "\r\r" drops the second one: the host's
    (b"@a\nAC\n+\nII\n@b\nACGT\n+\nIII\n@c\nA\n+\nI\n", 1),                         # a quality string one byte short
    (b"@a\nAC\n+\nII\n@b\nACGT\n+\nIIIII\n@c\nA\n+\nI\n", 1),                       # ... one byte long
    (b"@a\nAC\n+\nII\n@b\nG\n+\nI", 1),                                            # the last record without its line break
    (b"@a\nAC\n+\nII\n@", 1),                                                      # the range ends behind a header character
    (b"@a\nAC\n+\nII\n@bc", 1),                                                    # ... inside a name
    (b"@a\nAC\n+\nII\n@b\nG\n+b", 1),                                              # ... inside a '+' line
    (b"@a\nAC\n+\nII\n@b\nG\n+\nI\n", 2),                                          # ... exactly behind a quality line's line break
    (b">a\nAC\n>", 1),
    (b">a\nAC\n", 0),
]


def check_hand_cases(lib):
    for data, want in HAND:
        check_scan(lib, data, want)
    assert len(TF.kseq_records(HAND[19][0])[0]) == 3 and len(TF.kseq_records(HAND[20][0])[0]) == 3      # (kseq itself reads on there)


def one_per_length(lens, fastq, eol=b"\n"):
    rng = np.random.default_rng(3)
    recs = [[b"r%d" % i, bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), l)), bytes(rng.integers(33, 127, l).astype(np.uint8))] for i, l in enumerate(lens)]
    return (TF.fastq_bytes if fastq else TF.fasta_bytes)(recs, 0, eol), len(recs)


def check_seeded(lib):
    files = TF.seeded_files()
    for name, data in files.items():
        records = TF.kseq_records(data)[0]
        if name in ("fq_crlf", "fq_cr_last_byte"):                  # an empty read is a line "\r" there: the device stops at the first
            want = next(i for i, r in enumerate(records) if r[1] == b"\r")
        elif name.startswith("fa") or name in ("junk_in_front", "empty_lines", "fq_no_final_newline"):
            want = len(records) - 1                                 # the last record: no header behind it, or no line break
        else:
            want = len(records)
        assert check_scan(lib, data, want) == want and want > 0, name
    tile = LC.header_define("LQ_FXSCAN_TILE")
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, tile - 4, tile - 3, tile - 2, 2 * tile, 0, 0, 5]
    for fastq in (True, False):
        for eol in (b"\n", b"\r\n"):
            data, n = one_per_length(lens, fastq, eol)
            records = TF.kseq_records(data)[0]
            assert len(records) == n
            if eol == b"\r\n" and fastq:
                check_scan(lib, data, 0)                            # (the first read is empty: a line "\r")
                data, n = one_per_length([l for l in lens if l], fastq, eol)
            check_scan(lib, data, n if fastq else n - 1)
    # every record boundary of a 20-record file as the start
    recs = TF.rand_records(31, extra=6)
    assert len(recs) == 20
    fq, fa = TF.fastq_bytes(recs, 60), TF.fasta_bytes(recs, 60)
    at = [i for i in range(len(fq)) if fq[i:i + 2] == b"@r" and (i == 0 or fq[i - 1] == 10) and fq[i + 2:i + 3].isdigit()]
    starts = []
    for i in at:                                                   # (a quality line may start with "@r": keep the true headers)
        if not starts or len(TF.kseq_records(fq[i:])[0]) == 20 - len(starts):
            starts.append(i)
    assert len(starts) == 20
    for k, i in enumerate(starts):
        check_scan(lib, fq, 20 - k, pos=i, lc=0)
        check_scan(lib, fq, 20 - k, pos=i + 1, lc=ord("@"))
    starts = [i for i in range(len(fa)) if fa[i:i + 1] == b">" and (i == 0 or fa[i - 1] == 10)]
    assert len(starts) == 20
    for k, i in enumerate(starts):
        check_scan(lib, fa, 19 - k, pos=i, lc=0)
        check_scan(lib, fa, 19 - k, pos=i + 1, lc=ord(">"))
    # a start in the middle of a line gives nothing
    assert chunkpass.scan_records(fq, 1, 0, lib=lib)[0].shape[0] == 0 and chunkpass.scan_records(fq, 1, 0, lib=lib)[3] == (1, 0)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_scan_hand_cases(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_hand_cases(emu_lib)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_scan_seeded_files(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_seeded(emu_lib)


@pytest.mark.gpu
def test_gpu_scan_hand_cases(gpu_lib):
    check_hand_cases(gpu_lib)


@pytest.mark.gpu
def test_gpu_scan_seeded_files(gpu_lib):
    check_seeded(gpu_lib)

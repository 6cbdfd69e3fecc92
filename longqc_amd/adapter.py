"""The adapter search of LongQC's sampleqc (lq_adapt.py:10-101 `cut_adapter`, driven by longQC.py:285-292, 324-357, 508-517)
over the C ABI of include/lqcov.h (lqadapt_reads): the edit-distance part -- what `edlib.align(adapter, window, mode="HW",
task="path")` reports for the first / last `length` bases of a read -- runs on the device (kernels_adapt.hpp); the skip, the
identity test and the in-place trimming run here, in the reference's order.  No CPU fallback: without liblqcov.so or a HIP
device the calls raise.

What differs from lq_adapt.cut_adapter: an empty chunk gives (-1, 0, []) per adapter where the reference raises IndexError
at `reads[0]`; `length` must lie in [1, 4096]."""
import array
import ctypes as C
import logging
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import api

logger = logging.getLogger(__name__)


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqadapt_bound", False):
        lib.lqadapt_reads.restype = C.c_int
        lib.lqadapt_reads.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32,
                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib._lqadapt_bound = True
    return lib


def _bytes(s) -> bytes:
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def _hits(seqs: Sequence, adp5, adp3, length: int, device: int = 0, lib=None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """(n x 4 int32 of d, s, e, L for the 5' windows, the same for the 3' windows), None for an adapter not given.  Reads
    shorter than 2 * length get rows of -1.  Only the two windows of a read travel: a long read goes to the library as its
    first and last `length` bases (a read of exactly 2 * length, whose windows are those of the read)."""
    lib = _lib(lib)
    if not 1 <= length <= 4096:
        raise ValueError("length must lie in [1, 4096]")
    n = len(seqs)
    two = 2 * length
    parts = [s[:length] + s[-length:] if len(s) >= two else s[:0] for s in seqs]
    lens = np.fromiter((len(p) for p in parts), dtype=np.uint64, count=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = "".join(parts).encode("latin-1") if n and isinstance(parts[0], str) else b"".join(_bytes(p) for p in parts)
    if len(flat) != int(off[n]):
        raise ValueError("reads must be all str or all bytes")
    a5, a3 = (_bytes(adp5) if adp5 else None), (_bytes(adp3) if adp3 else None)
    o5 = np.empty((max(n, 1), 4), dtype=np.int32) if a5 else None
    o3 = np.empty((max(n, 1), 4), dtype=np.int32) if a3 else None
    err = C.create_string_buffer(512)
    rc = lib.lqadapt_reads(device, n, flat if n else None, off.ctypes.data, a5, len(a5) if a5 else 0, a3, len(a3) if a3 else 0,
                           length, o5.ctypes.data if a5 else None, o3.ctypes.data if a3 else None, err, 512)
    if rc != 0:
        raise api.LqcovError(rc, err.value.decode())
    return (o5[:n] if a5 else None), (o3[:n] if a3 else None)


def adapter_hits(seqs: Sequence, adp, length: int = 150, which: int = 5, device: int = 0, lib=None) -> np.ndarray:
    """Per read, (d, s, e, L) of edlib.align(adp, seq[:length] (which=5) or seq[-length:] (which=3), mode="HW", task="path"):
    edit distance, locations[0] and the summed CIGAR length; rows of -1 for reads shorter than 2 * length (never aligned)."""
    if which not in (5, 3):
        raise ValueError("which must be 5 or 3")
    o5, o3 = _hits(seqs, adp if which == 5 else None, adp if which == 3 else None, length, device, lib)
    return o5 if which == 5 else o3


def _identity(rows: np.ndarray) -> np.ndarray:
    """lq_adapt.py:30,63: 1.0 - d / L in double (true division of two integers: the correctly rounded quotient, as in Python)"""
    return 1.0 - rows[:, 0].astype(np.float64) / np.maximum(rows[:, 3], 1).astype(np.float64)


def _cut(reads, rows, th, r, three, len_list, lens):
    """_cutf (three=False, lq_adapt.py:45-78) / _cutr (three=True, :10-43) on rows computed for the untrimmed reads.
    reads None: nothing to trim, the tuple alone (it needs the rows and the lengths only)."""
    has_qual = len(reads[0]) > 2 if reads else False
    if len_list:                                                   # (only a non-empty list is appended to)
        len_list.extend(int(x) for x in lens)
    ok = lens >= 2 * r
    skip_num = int(np.count_nonzero(~ok))
    ident = _identity(rows)
    hit = np.flatnonzero(ok & (ident > th))
    iden_max = float(ident[hit].max()) if hit.size else -1
    cut_pos = []
    if reads is None:
        cut_pos = (r - rows[hit, 1].astype(np.int64)).tolist() if three else rows[hit, 2].astype(np.int64).tolist()
        hit = hit[:0]
    for i in hit.tolist():
        read = reads[i]
        if three:
            s = int(rows[i, 1])
            cut_pos.append(r - s)
            start = len(read[1]) - r + s
            read[1] = read[1][:start]
            if has_qual:
                read[2] = read[2][:start]
        else:
            e = int(rows[i, 2])
            cut_pos.append(e)
            read[1] = read[1][e + 1:]
            if has_qual:
                read[2] = read[2][e + 1:]
    logger.info("%d reads were skipped due to their short lengths." % skip_num)
    return (iden_max, len(cut_pos), cut_pos)


def trim_bounds(o5, o3, lens, th=0.75, length=150):
    """What _cut leaves of every read, in the untrimmed read's coordinates: (begin, end) as uint32 arrays, read i keeps
    seq[begin[i]:end[i]].  o5 / o3: the rows of the 5' / 3' search (n x 4 of d, s, e, L; None: that adapter is not cut), lens: the
    reads' lengths.  begin = e5 + 1 where the read is long enough (>= 2 * length) and the 5' identity exceeds th, else 0; end =
    L - length + s3 where the identity exceeds th and the 5'-trimmed read is long enough (L - begin >= 2 * length), else L."""
    lens = np.asarray(lens, dtype=np.int64)
    begin, end = np.zeros(lens.shape[0], dtype=np.int64), lens.copy()
    if o5 is not None:
        hit = (lens >= 2 * length) & (_identity(o5) > th)
        begin[hit] = o5[hit, 2].astype(np.int64) + 1
    if o3 is not None:
        hit = (lens - begin >= 2 * length) & (_identity(o3) > th)
        end[hit] = lens[hit] - length + o3[hit, 1].astype(np.int64)
    return begin.astype(np.uint32), end.astype(np.uint32)


def cut_adapter(reads, len_list=None, adp_t=None, adp_b=None, th=0.75, length=150, device=0, lib=None, chunk=None, bounds_out=None):
    """== lq_adapt.cut_adapter (lq_adapt.py:80-101): reads are LongQC's mutable [name, seq, qual, ...] records, trimmed in
    place; returns (iden_max, match_num, cut_pos) for one adapter, ((...5'), (...3')) for two, None (logged) for none.
    chunk: a chunkpass.ReadChunk made of these (untrimmed) reads: the search runs on its device copy, which stays as it is;
    nothing is gathered or uploaded.  With a chunk, reads may be None: the tuples alone, no record is trimmed.
    bounds_out: a list that is given [begin, end], trim_bounds of the rows this call searched (what a FastqWriter takes)."""
    if not adp_t and not adp_b:
        logger.error("No adapter sequence is given.")
        return None
    if chunk is not None:
        if not 1 <= length <= 4096:
            raise ValueError("length must lie in [1, 4096]")
        if reads is not None and len(reads) != chunk.n:
            raise ValueError("the chunk does not hold these reads")
        o5, o3 = chunk.adapt(_bytes(adp_t) if adp_t else None, _bytes(adp_b) if adp_b else None, length)
        lens = chunk.lens.copy()
    else:
        seqs = [rd[1] for rd in reads]
        o5, o3 = _hits(seqs, adp_t, adp_b, length, device, lib)
        lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    if bounds_out is not None:
        bounds_out[:] = trim_bounds(o5, o3, lens, th, length)
    t5 = t3 = None
    if adp_t:
        t5 = _cut(reads, o5, th, length, False, len_list, lens)
        logger.info("Adapter Sequence: %s, max identity:%f and the number of trimmed reads: %d" % (adp_t, t5[0], t5[1]))
        if adp_b:                                                  # the 3' skip test sees the 5'-trimmed length
            lens = lens.copy()
            hit5 = np.zeros(lens.shape[0], dtype=bool)
            ok5 = lens >= 2 * length
            hit5[ok5] = _identity(o5[ok5]) > th
            lens[hit5] -= o5[hit5, 2].astype(np.int64) + 1
    if adp_b:
        t3 = _cut(reads, o3, th, length, True, None if adp_t else len_list, lens)
        logger.info("Adapter Sequence: %s, max identity:%f and the number of trimmed reads: %d" % (adp_b, t3[0], t3[1]))
    if adp_t and adp_b:
        return (t5, t3)
    return t5 if adp_t else t3


class AdapterStats:
    """The run-level bookkeeping of longQC.py around cut_adapter: the variables of :285-292, the per-chunk update of :348-357
    and the `Stats_for_adapter5/3` blocks of :508-517 (written only when the maximum identity reaches 0.75)."""

    def __init__(self, adp5=None, adp3=None):
        self.adp5, self.adp3 = adp5, adp3
        self.num_trim5, self.max_iden_adp5, self.adp_pos5 = 0, 0.0, array.array('i')
        self.num_trim3, self.max_iden_adp3, self.adp_pos3 = 0, 0.0, array.array('i')

    def add(self, result) -> None:
        """one chunk's cut_adapter(...) result, as cut_adapter returned it for the adapters given here"""
        tuple_5 = tuple_3 = None
        if self.adp5 and self.adp3:
            tuple_5, tuple_3 = result
        elif self.adp5:
            tuple_5 = result
        elif self.adp3:
            tuple_3 = result
        if self.adp5 and tuple_5:
            if tuple_5[0] > self.max_iden_adp5:
                self.max_iden_adp5 = tuple_5[0]
            self.num_trim5 += tuple_5[1]
            self.adp_pos5.fromlist(tuple_5[2])
        if self.adp3 and tuple_3:
            if tuple_3[0] > self.max_iden_adp3:
                self.max_iden_adp3 = tuple_3[0]
            self.num_trim3 += tuple_3[1]
            self.adp_pos3.fromlist(tuple_3[2])

    def json_block(self) -> dict:
        out = {}
        if self.adp5 and self.max_iden_adp5 >= 0.75:
            out["Stats_for_adapter5"] = {"Num_of_trimmed_reads_5": self.num_trim5, "Max_identity_adp5": self.max_iden_adp5,
                                         "Average_position_from_5_end": np.mean(self.adp_pos5)}
        if self.adp3 and self.max_iden_adp3 >= 0.75:
            out["Stats_for_adapter3"] = {"Num_of_trimmed_reads_3": self.num_trim3, "Max_identity_adp3": self.max_iden_adp3,
                                         "Average_position_from_3_end": np.mean(self.adp_pos3)}
        return out

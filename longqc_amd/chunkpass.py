"""One upload per chunk: the chunk loop of `longQC.py sampleqc` (longQC.py:299-360) and the coverage call (:438-445) on the same
device bytes, over the lqchunk_* / lqstore_* calls of include/lqcov.h.

FileChunks is the loop's source, lq_utils.open_seq_chunk for a plain or gzip FASTA/FASTQ file or an unaligned BAM (lqreader_*): it yields
(chunk, n_seqs, n_bases) with `chunk` a ReadChunk that the library filled on the device straight from the file -- no read is a Python
object, the bases are never on the host.  SampleQCPass.run_file(path) is the whole loop on such chunks.

ReadChunk gathers a chunk's [name, seq, qual] records into flat arrays once and uploads them once; sdust.sdust_rows,
adapter.cut_adapter and LqGCMI355X.calc_read_and_chunk_gc_frac take it as `chunk=` and then run on the device copy.
SampleQCPass is the loop's body and the coverage call: add_chunk(reads) per chunk -- low-complexity rows, adapter search,
subsample, GC fractions, then the chunk is 2-bit packed on the device and kept there -- and coverage(), which maps the subsample
against the kept chunks without touching the input again.  No CPU fallback: without liblqcov.so or a HIP device the calls raise."""
import ctypes as C
import io
import math
import os
import sys
from typing import Optional

import numpy as np

from . import adapter, api, gcfrac, sampleqc, sdust


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqchunk_bound", False):
        H, P = C.c_void_p, C.c_void_p
        sig = {
            "lqchunk_create": (H, [C.c_int]),
            "lqchunk_destroy": (None, [H]),
            "lqchunk_last_error": (C.c_char_p, [H]),
            "lqchunk_load": (C.c_int, [H, C.c_uint32, P, P, P]),
            "lqchunk_sdust": (C.c_int, [H, C.c_int, C.c_int, P, P, P]),
            "lqchunk_sdust_split": (C.c_int, [H, C.c_int, C.c_int, C.c_uint32, P, P, P, P]),
            "lqchunk_sdust_table": (C.c_int, [H, C.c_char_p, P, P, C.c_uint64, P, P, P, C.c_uint64]),
            "lqchunk_sdust_columns": (C.c_int, [H, P, P]),
            "lqchunk_sdust_intervals": (C.c_int, [H, C.c_int, C.c_int, C.c_uint32, P, P, P, C.c_size_t, P]),
            "lqchunk_adapt": (C.c_int, [H, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, P, P]),
            "lqchunk_gc": (C.c_int, [H, C.c_uint32, P, P, P, C.c_uint64, C.c_uint64, P, P, P, P]),
            "lqchunk_pack": (C.c_int, [H]),
            "lqchunk_get_packed": (C.c_int, [H, P, P, P]),
            "lqstore_create": (H, [C.c_int]),
            "lqstore_destroy": (None, [H]),
            "lqstore_append": (C.c_int, [H, H, C.c_char_p, P]),
            "lqstore_bytes": (C.c_uint64, [H]),
            "lqstore_run": (C.c_int, [H, H]),
            "lqchunk_get_reads": (C.c_int, [H, C.c_uint32, P, P, P]),
            "lqreader_open": (H, [C.c_char_p, C.c_int, C.c_uint64, C.c_int, C.c_uint32, C.c_int]),
            "lqreader_next": (C.c_int, [H, H, P, P, P, P]),
            "lqreader_names": (C.c_int, [H, P, P, P]),
            "lqreader_close": (None, [H]),
            "lqreader_last_error": (C.c_char_p, [H]),
            "lqreader_format": (C.c_int, [H]),
            "lqreader_bam_qualities": (C.c_int, [H, C.c_int]),
            "lqreader_inflate": (C.c_int, [H, C.c_int]),
            "lqinflate_blocks": (C.c_int, [C.c_int, P, C.c_uint64, C.c_uint32, P, P, P, P, P, P]),
            "lqinflate_gzip": (C.c_int, [C.c_int, P, C.c_uint64, C.c_uint32, P, C.c_uint64, P, P]),
            "lqreader_inflate_stats": (C.c_int, [H, P]),
            "lqreader_parse": (C.c_int, [H, C.c_int]),
            "lqreader_parse_stats": (C.c_int, [H, P]),
            "lqfx_scan": (C.c_int, [C.c_int, P, C.c_uint64, C.c_uint64, C.c_int, P, C.c_uint64, P, P, C.c_uint64, P, P, P, P, P]),
            "lqreader_host_copy": (C.c_int, [H, C.c_int]),
            "lqreader_bam_walk": (C.c_int, [H, C.c_int]),
            "lqbam_scan": (C.c_int, [C.c_int, P, C.c_uint64, C.c_uint64, C.c_int, P, C.c_uint64, P, P, C.c_uint64, P, P, P, P]),
            "lqreader_copy_stats": (C.c_int, [H, P]),
            "lqcrc32_ranges": (C.c_int, [C.c_int, P, C.c_uint64, C.c_uint32, P, P, P]),
            "lqfx_names": (C.c_int, [C.c_int, P, C.c_uint64, P, C.c_uint64, P, C.c_uint64, P, P]),
            "lqchunk_fastq": (C.c_int, [H, C.c_char_p, P, P, P, P, C.c_uint64, P]),
            "lqfastq_open": (H, [C.c_char_p, C.c_int, C.c_uint64]),
            "lqfastq_write": (C.c_int, [H, H, C.c_char_p, P, P, P, P]),
            "lqfastq_close": (C.c_int, [H]),
            "lqfastq_last_error": (C.c_char_p, [H]),
            "lqfastq_kernel_ms": (C.c_double, [H]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib._lqchunk_bound = True
    return lib


def _join(items, n):
    """one buffer of all items (all str or all bytes) and their lengths"""
    lens = np.fromiter((len(s) for s in items), dtype=np.int64, count=n)
    flat = "".join(items).encode("latin-1") if n and isinstance(items[0], str) else b"".join(items)
    if len(flat) != int(lens.sum()):
        raise ValueError("reads must be all str or all bytes")
    return flat, lens


INFLATE_MODES = {"host": 0, "device": 1}
INFLATE_OK, INFLATE_INVALID, INFLATE_INPUT, INFLATE_LONG, INFLATE_SHORT = range(5)      # lqinflate_blocks' status words


def inflate_mode(inflate):
    """"host" | "device" | None (the environment variable LQREADER_INFLATE, "host" without it) -> the mode's name"""
    mode = os.environ.get("LQREADER_INFLATE", "host") if inflate is None else inflate
    if mode not in INFLATE_MODES:
        raise ValueError("inflate must be 'host' or 'device', not %r" % (mode,))
    return mode


def inflate_blocks(comp, in_off, in_len, out_off, isize, out=None, device: int = 0, lib=None):
    """k_bgzf_inflate over arrays (lqinflate_blocks): block i is the raw deflate stream comp[in_off[i] : in_off[i] + in_len[i]] and
    inflates to out[out_off[i] : out_off[i] + isize[i]] (isize <= 65536).  out: a uint8 array to write into (what lies outside the
    blocks' ranges stays), default zeros up to the last range's end.  -> (out, status uint32[n]: INFLATE_OK, INFLATE_INVALID and
    INFLATE_INPUT (not a whole deflate stream), INFLATE_LONG and INFLATE_SHORT (a stream of more / fewer bytes than isize))"""
    lib = _lib(lib)
    comp = np.frombuffer(bytes(comp), dtype=np.uint8) if not isinstance(comp, np.ndarray) else np.ascontiguousarray(comp, dtype=np.uint8)
    in_off, out_off = np.ascontiguousarray(in_off, dtype=np.uint64), np.ascontiguousarray(out_off, dtype=np.uint64)
    in_len, isize = np.ascontiguousarray(in_len, dtype=np.uint32), np.ascontiguousarray(isize, dtype=np.uint32)
    n = in_off.shape[0]
    if not (in_len.shape[0] == out_off.shape[0] == isize.shape[0] == n):
        raise ValueError("in_off, in_len, out_off and isize differ in length")
    end = int((out_off + isize.astype(np.uint64)).max()) if n else 0
    if out is None:
        out = np.zeros(end, np.uint8)
    if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.shape[0] < end:
        raise ValueError("out must be a contiguous uint8 array that holds every block's range")
    status = np.zeros(max(n, 1), np.uint32)
    rc = lib.lqinflate_blocks(device, comp.ctypes.data if comp.shape[0] else None, comp.shape[0], n, in_off.ctypes.data, in_len.ctypes.data,
                              out_off.ctypes.data, isize.ctypes.data, out.ctypes.data if out.shape[0] else None, status.ctypes.data)
    if rc != 0:
        raise api.LqcovError(rc, lib.lqreader_last_error(None).decode())
    return out, status[:n]


INFLATE_STATS = ("launches", "spans_found", "spans_accepted", "spans_rejected", "markers_resolved", "bytes_device", "bytes_zlib")


def _stats_dict(words):
    return dict(zip(INFLATE_STATS, (int(w) for w in words)))


def inflate_gzip(data, span_bytes: Optional[int] = None, device: int = 0, lib=None, out_cap: Optional[int] = None):
    """A whole gzip file in memory, inflated on the device by speculative spans (lqinflate_gzip: k_gz_find, k_gz_inflate_spec,
    k_gz_window, k_gz_resolve; zlib on the host for what the device cannot vouch for).  span_bytes: compressed bytes per span, a
    multiple of 16 from 1024 to 131072, None: LQREADER_GZ_SPAN_BYTES or the default.  out_cap: room for the bytes, default what the
    members' ISIZE fields and the deflate bound allow.  -> (bytes, stats: a dict of INFLATE_STATS).  A stream that gzread would
    refuse raises LqcovError (-2)."""
    lib = _lib(lib)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    if out_cap is None:
        out_cap = 1032 * comp.shape[0] + 64                        # (deflate gives at most 1032 bytes per byte)
        if comp.shape[0] >= 18 and comp.shape[0] < (1 << 32):
            import zlib
            try:                                                    # (a well-formed file says how long it is)
                d, n, rest = zlib.decompressobj(31), 0, bytes(data)
                while rest[:2] == b"\x1f\x8b":
                    n += len(d.decompress(rest)); rest = d.unused_data
                    if not d.eof:
                        break
                    d = zlib.decompressobj(31)
                out_cap = n + 64
            except zlib.error:
                out_cap = min(out_cap, 1 << 28)
    out = np.empty(max(int(out_cap), 1), np.uint8)
    n, st = C.c_uint64(), (C.c_uint64 * len(INFLATE_STATS))()
    rc = lib.lqinflate_gzip(device, comp.ctypes.data if comp.shape[0] else None, comp.shape[0], int(span_bytes or 0), out.ctypes.data, int(out_cap),
                            C.byref(n), st)
    if rc != 0:
        raise api.LqcovError(rc, lib.lqreader_last_error(None).decode())
    return out[:n.value].tobytes(), _stats_dict(st)


split_mode = sdust.split_mode                                       # "serial" | "pieces" | None (LQSDUST_SPLIT): how ReadChunk.sdust scans long reads


def _piece(piece):
    """piece as the C ABI takes it: 0 for None (the default), else the number of bases, which must fit 32 bits"""
    p = int(piece or 0)
    if not 0 <= p <= 0xffffffff:
        raise ValueError("piece must be None or a number of bases from 0 to 2^32 - 1, not %r" % (piece,))
    return p


PARSE_MODES = {"host": 0, "device": 1}
PARSE_STATS = ("pieces", "scans", "records_device", "records_host", "lines", "fallbacks")
GATHER_FILL = 0xffffffffffffffff                                    # src of a quality segment without source bytes ('!')


def parse_mode(parse):
    """"host" | "device" | None (the environment variable LQREADER_PARSE, "host" without it) -> the mode's name"""
    mode = os.environ.get("LQREADER_PARSE", "host") if parse is None else parse
    if mode not in PARSE_MODES:
        raise ValueError("parse must be 'host' or 'device', not %r" % (mode,))
    return mode


def scan_records(data, start_pos: int = 0, last_char: int = 0, device: int = 0, lib=None):
    """The record scan of the reader's device mode over bytes in memory (lqfx_scan: k_fx_lines, k_fx_candidates, k_fx_jump, k_fx_emit).
    A kseq parser stands at data[start_pos] with last_char (0, or ord("@") / ord(">"): the header character data[start_pos - 1] has
    been consumed).  -> (rows uint32[n, 4]: name offset, name length, sequence length, flags (bit 0: a quality string) of every
    record the device vouches for, in file order; sseg, qseg uint64[k, 2]: (src, dst) of every line of the sequences / quality
    strings that gives bytes, src GATHER_FILL for a record without qualities; resume = (pos, last_char) behind the last row)"""
    lib = _lib(lib)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.shape[0]
    cap = n // 2 + 2
    rows, sseg, qseg = np.zeros((cap, 4), np.uint32), np.zeros((cap, 2), np.uint64), np.zeros((cap, 2), np.uint64)
    n_rows, n_s, n_q, r_pos, r_lc = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    rc = lib.lqfx_scan(device, buf.ctypes.data if n else None, n, int(start_pos), int(last_char), rows.ctypes.data, cap, sseg.ctypes.data,
                       qseg.ctypes.data, cap, C.byref(n_rows), C.byref(n_s), C.byref(n_q), C.byref(r_pos), C.byref(r_lc))
    if rc != 0:
        raise api.LqcovError(rc, lib.lqreader_last_error(None).decode())
    return rows[:n_rows.value].copy(), sseg[:n_s.value].copy(), qseg[:n_q.value].copy(), (r_pos.value, r_lc.value)


BAMWALK_MODES = {"host": 0, "device": 1}


def bam_walk_mode(bam_walk):
    """"host" | "device" | None (the environment variable LQREADER_BAMWALK, "host" without it) -> the mode's name"""
    mode = os.environ.get("LQREADER_BAMWALK", "host") if bam_walk is None else bam_walk
    if mode not in BAMWALK_MODES:
        raise ValueError("bam_walk must be 'host' or 'device', not %r" % (mode,))
    return mode


def scan_bam_records(data, start_pos: int = 0, with_qual: bool = False, device: int = 0, lib=None):
    """The record walk of an unaligned BAM on the device over bytes in memory (lqbam_scan: k_bam_candidates, k_bam_link, k_fx_jump,
    k_bam_emit).  data: inflated BAM bytes; a parser stands at data[start_pos], a record boundary behind the BAM header.  -> (rows
    uint32[n, 4]: name offset, name length (up to the first NUL), l_seq, flags (bit 0: with_qual) of every record the device vouches
    for, in file order; sseg, qseg uint64[k, 2]: (src, dst) per record with bases -- src the first byte of the packed sequence / of
    the quality bytes, GATHER_FILL without with_qual; resume: the first offset of the chain that is not vouched, or len(data))"""
    lib = _lib(lib)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.shape[0]
    cap = n // 36 + 2
    rows, sseg, qseg = np.zeros((cap, 4), np.uint32), np.zeros((cap, 2), np.uint64), np.zeros((cap, 2), np.uint64)
    n_rows, n_s, n_q, r_pos = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib.lqbam_scan(device, buf.ctypes.data if n else None, n, int(start_pos), int(bool(with_qual)), rows.ctypes.data, cap, sseg.ctypes.data,
                        qseg.ctypes.data, cap, C.byref(n_rows), C.byref(n_s), C.byref(n_q), C.byref(r_pos))
    if rc != 0:
        raise api.LqcovError(rc, lib.lqreader_last_error(None).decode())
    return rows[:n_rows.value].copy(), sseg[:n_s.value].copy(), qseg[:n_q.value].copy(), r_pos.value


HOSTCOPY_MODES = {"all": 0, "needed": 1}
COPY_STATS = ("active", "bytes_inflated", "bytes_to_host", "bytes_crc_device", "bytes_crc_host", "names_device")


def host_copy_mode(host_copy):
    """"all" | "needed" | None (the environment variable LQREADER_HOSTCOPY, "all" without it) -> the mode's name"""
    mode = os.environ.get("LQREADER_HOSTCOPY", "all") if host_copy is None else host_copy
    if mode not in HOSTCOPY_MODES:
        raise ValueError("host_copy must be 'all' or 'needed', not %r" % (mode,))
    return mode


def crc32_ranges(data, off, length, device: int = 0, lib=None):
    """zlib.crc32 of data[off[i] : off[i] + length[i]] for every i, made on the device (lqcrc32_ranges: k_crc32_ranges).  The ranges may
    start anywhere, have any length, touch and overlap; an empty range gives 0.  -> uint32[n].  A range outside data raises LqcovError
    (-1)."""
    lib = _lib(lib)
    buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off, length = np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(length, dtype=np.uint64)
    n = off.shape[0]
    if length.shape[0] != n:
        raise ValueError("off and length differ in length")
    out = np.zeros(max(n, 1), np.uint32)
    rc = lib.lqcrc32_ranges(device, buf.ctypes.data if buf.shape[0] else None, buf.shape[0], n, off.ctypes.data, length.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise api.LqcovError(rc, lib.lqreader_last_error(None).decode())
    return out[:n]


def gather_names(data, rows, device: int = 0, lib=None):
    """The names of scan_records' rows, gathered on the device (lqfx_names: k_fx_names): -> (blob: every name followed by one NUL,
    bytes; name_off uint64[n + 1]: where each starts, the last one the blob's length; first_bad: the first row whose name holds a
    byte of 0x80 or more, n if none)"""
    lib = _lib(lib)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 4)
    n = rows.shape[0]
    cap = int(rows[:, 1].astype(np.uint64).sum()) + n
    names, name_off, first_bad = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.uint64), C.c_uint64()
    rc = lib.lqfx_names(device, buf.ctypes.data if buf.shape[0] else None, buf.shape[0], rows.ctypes.data if n else None, n, names.ctypes.data, cap,
                        name_off.ctypes.data, C.byref(first_bad))
    if rc != 0:
        raise api.LqcovError(rc, lib.lqreader_last_error(None).decode())
    return names[:int(name_off[n])].tobytes(), name_off, int(first_bad.value)


class ReadChunk:
    """A chunk of LongQC's [name, seq, qual, ...] records on the device.  n, names, lens (int64), off (uint64, n + 1) describe it on
    the host; the records themselves are not kept.  load(reads) puts another chunk into the same handle, whose device buffers
    are used again and grow.  reads=None: an empty handle, for FileChunks to fill.  records(idx) brings reads back as lists."""

    def __init__(self, reads, device: int = 0, lib=None):
        self.lib = _lib(lib)
        self.device = device
        self.h = self.lib.lqchunk_create(device)
        if not self.h:
            raise api.LqcovError(-3, self.lib.lqchunk_last_error(None).decode() or "lqchunk_create failed (no HIP device?)")
        self.n, self.names, self.lens, self.off = 0, [], np.zeros(0, np.int64), np.zeros(1, np.uint64)
        self.n_serial = 0                                           # reads of the last sdust(split="pieces") that took the serial walk
        self.qflat, self.packed, self.from_file, self._name_blob = None, False, False, None
        if reads is not None:
            self.load(reads)

    def load(self, reads):
        n = self.n = len(reads)
        self.packed, self.from_file, self._name_blob = False, False, None
        self.names = [r[0].decode() if isinstance(r[0], (bytes, bytearray)) else str(r[0]) for r in reads]
        self.flat, self.lens = _join([r[1] for r in reads], n)
        self.off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(self.lens, out=self.off[1:])
        self.qflat = None
        quals = [r[2] if len(r) > 2 and r[2] else None for r in reads]
        if any(q is not None for q in quals):                      # reads without qualities: zero bytes, as lqsdust_reads takes them
            zero = "\0" if isinstance(next(q for q in quals if q is not None), str) else b"\0"
            self.qflat, qlens = _join([q if q is not None else zero * int(l) for q, l in zip(quals, self.lens)], n)
            if (qlens != self.lens).any():
                raise ValueError("a quality string differs in length from its read")
        self._ck(self.lib.lqchunk_load(self.h, n, self.flat if len(self.flat) else None, self.off.ctypes.data, self.qflat))

    def load_arrays(self, names, seq, off, qual=None):
        """load() for reads that are arrays already: seq (uint8) holds read i's bases at [off[i], off[i + 1]) (off: n + 1 offsets from 0),
        qual (uint8, as long as seq; None: no qualities) its qualities, a zero byte first for a read without.  No record becomes a string"""
        n = len(names)
        seq, off = np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
        qual = np.ascontiguousarray(qual, dtype=np.uint8) if qual is not None else None
        if off.shape != (n + 1,) or int(off[0]) != 0 or (n and (np.diff(off.astype(np.int64)) < 0).any()) or seq.shape != (int(off[n]),):
            raise ValueError("off holds n + 1 ascending offsets from 0 to the bases' number")
        if qual is not None and qual.shape != seq.shape:
            raise ValueError("a quality string differs in length from its read")
        self.n, self.names, self.off, self.lens = n, list(names), off, np.diff(off.astype(np.int64))
        self.packed, self.from_file, self._name_blob = False, False, None
        self.flat, self.qflat = seq, qual
        self._ck(self.lib.lqchunk_load(self.h, n, seq.ctypes.data if seq.size else None, off.ctypes.data, qual.ctypes.data if qual is not None and qual.size else None))

    def __len__(self):
        return self.n

    def _ck(self, rc: int):
        if rc != 0:
            raise api.LqcovError(rc, self.lib.lqchunk_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.lqchunk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _from_reader(self, reader, n: int):
        """the chunk lqreader_next has just put into the handle: names, lengths and offsets from lqreader_names"""
        names, noff, lens = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self.lib.lqreader_names(reader, C.byref(names), C.byref(noff), C.byref(lens)) != 0:
            raise api.LqcovError(-1, "lqreader_names failed")
        self.n, self.packed, self.from_file, self.flat, self.qflat = n, False, True, None, None
        name_off = np.ctypeslib.as_array(C.cast(noff, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        blob = C.string_at(names, int(name_off[n]))
        self._name_blob = (blob, name_off)                          # as lqstore_append takes them
        self.names = blob.decode("ascii").split("\0")[:n]
        self.lens = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint32)), (n,)).astype(np.int64) if n else np.zeros(0, np.int64)
        self.off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(self.lens, out=self.off[1:])

    def qual_array(self) -> Optional[np.ndarray]:
        return None if self.qflat is None else np.frombuffer(self.qflat, dtype=np.uint8)

    def qual_first(self):
        """what sdust._rows asks the qualities: the host copy (its first byte per read tells whether the read has any), None without
        qualities, True for a chunk read from a file -- there every read with bases has qualities ('!' where the file had none), and
        they are on the device only"""
        return True if self.from_file else self.qual_array()

    def records(self, idx=None):
        """-> [name, seq, qual] lists (str; [name, seq] for a chunk loaded without qualities) of the reads `idx` (default: all), copied
        back from the device: lqchunk_get_reads"""
        idx = np.arange(self.n, dtype=np.uint32) if idx is None else np.ascontiguousarray(idx, dtype=np.uint32)
        with_qual = self.from_file or self.qflat is not None
        lens = self.lens[idx.astype(np.int64)] if idx.size else np.zeros(0, np.int64)
        total = int(lens.sum())
        seq = np.empty(max(total, 1), np.uint8)
        qual = np.empty(max(total, 1), np.uint8) if with_qual else None
        self._ck(self.lib.lqchunk_get_reads(self.h, idx.size, idx.ctypes.data if idx.size else None, seq.ctypes.data,
                                            qual.ctypes.data if with_qual else None) if idx.size else 0)
        s = seq[:total].tobytes().decode("latin-1")
        q = qual[:total].tobytes().decode("latin-1") if with_qual else None
        out, a = [], 0
        for i, l in zip(idx.tolist(), lens.tolist()):
            out.append([self.names[i], s[a:a + l], q[a:a + l]] if with_qual else [self.names[i], s[a:a + l]])
            a += l
        return out

    def names_c(self):
        """the names as the C ABI takes them (NUL-terminated blob, uint64 offsets), encoded once per chunk"""
        if self._name_blob is None:
            self._name_blob = api.encode_names(self.names)
        return self._name_blob

    def bounds_c(self, begin, end):
        """begin / end of fastq_bytes and FastqWriter.write as contiguous uint32 arrays of n entries, (None, None) for whole reads"""
        if (begin is None) != (end is None):
            raise ValueError("begin and end come together")
        if begin is None:
            return None, None
        begin, end = np.ascontiguousarray(begin, dtype=np.uint32), np.ascontiguousarray(end, dtype=np.uint32)
        if begin.shape != (self.n,) or end.shape != (self.n,):
            raise ValueError("begin and end must have one entry per read")
        return begin, end

    def fastq_bytes(self, begin=None, end=None) -> bytes:
        """the chunk's reads, read i cut to [begin[i], end[i]) (None: whole reads), as FASTQ text -- what sampleqc.write_fastq writes for
        records() trimmed that way -- made on the device (k_fastq_format): lqchunk_fastq"""
        begin, end = self.bounds_c(begin, end)
        nb, noff = self.names_c()
        kept = self.lens if begin is None else end.astype(np.int64) - begin.astype(np.int64)
        cap = int((np.diff(noff).astype(np.int64) - 1).sum() + 2 * kept.sum() + 6 * self.n) if self.n else 0
        out, n = np.empty(max(cap, 1), np.uint8), C.c_uint64()
        self._ck(self.lib.lqchunk_fastq(self.h, nb, noff.ctypes.data, begin.ctypes.data if begin is not None else None,
                                        end.ctypes.data if end is not None else None, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].tobytes()

    # -- the steps, as arrays --
    def sdust(self, w: int = 64, t: int = 20, split: Optional[str] = None, piece: Optional[int] = None):
        """-> (masked bases, sums of 10^(-q/10), qualities above Q7) per read: lqchunk_sdust.  split (split_mode's) "pieces": the same
        arrays from lqchunk_sdust_split -- reads of A/C/G/T alone are cut into pieces of `piece` bases (None: the default, 4096; at least
        2 w + 2) that are scanned side by side; n_serial then says how many reads took the serial walk all the same"""
        n = self.n
        masked, psum, qv = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint32)
        if split_mode(split) == "pieces":
            ns = C.c_uint32()
            self._ck(self.lib.lqchunk_sdust_split(self.h, w, t, _piece(piece), masked.ctypes.data, psum.ctypes.data, qv.ctypes.data, C.byref(ns)))
            self.n_serial = ns.value
        else:
            self._ck(self.lib.lqchunk_sdust(self.h, w, t, masked.ctypes.data, psum.ctypes.data, qv.ctypes.data))
        return masked, psum, qv

    def sdust_table(self, w: int = 64, t: int = 20, split: Optional[str] = None, piece: Optional[int] = None):
        """The chunk's low-complexity table as text, made on the device: the scan (lqchunk_sdust, or lqchunk_sdust_split with split
        "pieces") leaves its arrays there, lqchunk_sdust_table formats them (k_sdust_rows, k_sdust_text).  -> (bytes: the rows sdust._rows
        gives, each with its newline; stats: a dict of sdust.TABLE_STATS and exclude_first / exclude_second, the ascending indices of the
        reads on LongQC's two exclusion lists)"""
        if split_mode(split) == "pieces":
            ns = C.c_uint32()
            self._ck(self.lib.lqchunk_sdust_split(self.h, w, t, _piece(piece), None, None, None, C.byref(ns)))
            self.n_serial = ns.value
        else:
            self._ck(self.lib.lqchunk_sdust(self.h, w, t, None, None, None))
        return self.sdust_table_bytes()

    def sdust_table_bytes(self, out_cap: Optional[int] = None):
        """sdust_table's second half: the table of the last scan (lqchunk_sdust_table).  out_cap: room for the text, default what always
        suffices"""
        n = self.n
        nb, noff = self.names_c()
        cap = int((np.diff(noff).astype(np.int64) - 1).sum()) + sdust.ROW_FIELDS_MAX * n if out_cap is None else int(out_cap)
        out, n_out, st = np.empty(max(cap, 1), np.uint8), C.c_uint64(), (C.c_uint64 * len(sdust.TABLE_STATS))()
        excl = np.zeros(max(2 * n, 1), np.uint32)
        self._ck(self.lib.lqchunk_sdust_table(self.h, nb, noff.ctypes.data, out.ctypes.data, cap, C.byref(n_out), st, excl.ctypes.data, 2 * n))
        return out[:n_out.value].tobytes(), sdust.with_lists(sdust.stats_dict(st), excl)

    def sdust_columns(self):
        """The two "%.3f" columns of the table sdust_table / sdust_table_bytes made last, as the thousandths its text shows
        (lqchunk_sdust_columns) -> (fraction: uint32, 0xffffffff for "-nan"; meanQ: int32, figdata.MISSING for "-nan")"""
        frac, qv = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.int32)
        self._ck(self.lib.lqchunk_sdust_columns(self.h, frac.ctypes.data, qv.ctypes.data))
        return frac[:self.n], qv[:self.n]

    def sdust_intervals(self, w: int = 64, t: int = 20, piece: Optional[int] = None):
        """The masked intervals of the reads the pieces serve, what the reference's sdust() returns for them: lqchunk_sdust_intervals.
        -> (iv_off uint64[n + 1], iv uint64[k, 2]: (start, finish) of read i's intervals at iv[iv_off[i] : iv_off[i + 1]], ascending,
        disjoint and not adjacent; flagged bool[n]: the read holds a byte other than A/C/G/T and reports no interval -- only the serial
        walk can count such a read; reads of any length are served)"""
        n = self.n
        iv_off, flagged, need = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8), C.c_size_t()
        self._ck(self.lib.lqchunk_sdust_intervals(self.h, w, t, _piece(piece), iv_off.ctypes.data, flagged.ctypes.data, None, 0, C.byref(need)))
        iv = np.zeros(max(need.value, 1), np.uint64)
        self._ck(self.lib.lqchunk_sdust_intervals(self.h, w, t, _piece(piece), iv_off.ctypes.data, flagged.ctypes.data, iv.ctypes.data, need.value, C.byref(need)))
        iv = iv[:need.value]
        return iv_off, np.stack([iv >> np.uint64(32), iv & np.uint64(0xffffffff)], axis=1).astype(np.int64), flagged[:n].astype(bool)

    def adapt(self, adp5: Optional[bytes], adp3: Optional[bytes], length: int = 150):
        """-> (n x 4 int32 of d, s, e, L for the 5' windows, the same for the 3' windows), None for an adapter not given: lqchunk_adapt"""
        n = self.n
        o5 = np.empty((max(n, 1), 4), dtype=np.int32) if adp5 else None
        o3 = np.empty((max(n, 1), 4), dtype=np.int32) if adp3 else None
        self._ck(self.lib.lqchunk_adapt(self.h, adp5, len(adp5) if adp5 else 0, adp3, len(adp3) if adp3 else 0, length,
                                        o5.ctypes.data if adp5 else None, o3.ctypes.data if adp3 else None))
        return (o5[:n] if adp5 else None), (o3[:n] if adp3 else None)

    def gc(self, chunk_size, k, draw_off, pos_in, seed, first_read, gc, pos_out, win_gc, kept):
        """lqchunk_gc on caller-owned arrays (addresses or None), as gcfrac._call hands them over"""
        self._ck(self.lib.lqchunk_gc(self.h, chunk_size, k, draw_off, pos_in, seed, first_read, gc, pos_out, win_gc, kept))

    def pack(self):
        """2-bit pack the device copy on the device (k_chunk_pack): the layout of lqcov_pack_reads"""
        self._ck(self.lib.lqchunk_pack(self.h))
        self.packed = True

    def get_packed(self):
        """-> (codes uint64[4 * chunks], amb uint32[4 * chunks], flags uint8[n]) on the host"""
        if not self.packed:
            self.pack()
        nc = int(((self.lens + 127) // 128).sum())
        codes, amb, flags = np.zeros(max(nc, 1) * 4, np.uint64), np.zeros(max(nc, 1) * 4, np.uint32), np.zeros(max(self.n, 1), np.uint8)
        self._ck(self.lib.lqchunk_get_packed(self.h, codes.ctypes.data, amb.ctypes.data, flags.ctypes.data))
        return codes[:nc * 4], amb[:nc * 4], flags[:self.n]


class FileChunks:
    """lq_utils.open_seq_chunk(path, ..., is_upper, chunk_size) for a plain or gzip FASTA/FASTQ file, on the device: iterating yields
    (chunk, n_seqs, n_bases) -- chunk a ReadChunk filled from the file (n, names, lens, off, len(); records(idx) for the lists), n_seqs
    and n_bases cumulative over the file, and after the last record one more chunk, empty if the last record ended a chunk.  The chunk
    is the same object every time and valid until the next iteration: its handle's buffers are used again.  Every iteration starts
    the file anew.  str_overhead: sys.getsizeof("") of the interpreter whose chunk borders are wanted (49 or 41, by the CPython
    version; default: this interpreter's).
    A BAM file (parse_bam_chunk: every record a read, the name read_name, the sequence the decoded nibbles) is recognised by its
    first bytes; n_threads (default 16, at most 16) threads inflate its blocks.  is_sequel=True, what open_seq_chunk passes: every
    quality string is '!' * len; False: chr(q + 33) of the file's qualities.  `format` (0 FASTA/FASTQ, 1 BAM) is set when iteration
    starts.
    inflate="device": the BGZF blocks of a BAM file -- and of a bgzip FASTA/FASTQ, which otherwise is gzread's -- are inflated on the
    device (k_bgzf_inflate); "host": the thread pool and gzread; None: what the environment variable LQREADER_INFLATE says, "host"
    without it.  The chunks are the same.  A gzip file that is not BGZF is inflated in device mode by speculative spans (k_gz_*; the span
    length: LQREADER_GZ_SPAN_BYTES); inflate_stats (a dict of INFLATE_STATS) says after iteration what that took.
    parse="device": the records of a FASTA/FASTQ file are found on the device (k_fx_*, lqreader_parse) wherever it vouches for them,
    by the host parser elsewhere; "host": by the host parser; None: the environment variable LQREADER_PARSE, "host" without it.  The
    chunks are the same; parse_stats (a dict of PARSE_STATS) says after iteration who found what.  A BAM file ignores the mode.
    bam_walk="device": the records of a BAM file are found on the device (k_bam_*, lqreader_bam_walk) wherever it vouches for them --
    unaligned records that are whole inside a piece -- by the host walk elsewhere; "host": by the host walk; None: the environment
    variable LQREADER_BAMWALK, "host" without it.  The chunks are the same; parse_stats reports.  A FASTA/FASTQ file ignores the mode.
    host_copy="needed": where the device both inflates and parses a FASTA/FASTQ file, the inflated bytes stay there -- the members'
    CRC32 (k_crc32_ranges) and the names (k_fx_names) are made on the device and the host fetches only what its own parser must see;
    "all": every inflated byte comes back; None: the environment variable LQREADER_HOSTCOPY, "all" without it.  A BAM file honours
    it where the device both inflates and walks it (inflate and bam_walk "device").  Any other file or mode ignores it.  The chunks are the same; copy_stats (a dict of COPY_STATS) says after iteration what moved."""

    def __init__(self, path: str, chunk_size=0.5 * 1024 ** 3, is_upper: bool = True, device: int = 0, str_overhead: Optional[int] = None,
                 lib=None, n_threads: int = 0, is_sequel: bool = True, inflate: Optional[str] = None, parse: Optional[str] = None,
                 host_copy: Optional[str] = None, bam_walk: Optional[str] = None):
        self.lib = _lib(lib)
        self.bam_walk = bam_walk_mode(bam_walk)
        self.host_copy, self.copy_stats = host_copy_mode(host_copy), dict.fromkeys(COPY_STATS, 0)
        self.inflate = inflate_mode(inflate)
        self.parse, self.parse_stats = parse_mode(parse), dict.fromkeys(PARSE_STATS, 0)
        self.path, self.is_upper, self.device, self.n_threads = path, is_upper, device, n_threads
        self.is_sequel, self.format, self.inflate_stats = is_sequel, None, _stats_dict([0] * len(INFLATE_STATS))
        self.chunk_size = max(0, int(math.ceil(chunk_size)))        # size >= chunk_size for an integer size
        self.str_overhead = sys.getsizeof("") if str_overhead is None else int(str_overhead)

    def __iter__(self):
        lib = self.lib
        r = lib.lqreader_open(self.path.encode(), self.device, self.chunk_size, int(bool(self.is_upper)), self.str_overhead, self.n_threads)
        if not r:
            raise api.LqcovError(-2, lib.lqreader_last_error(None).decode() or "lqreader_open failed")
        chunk = None
        try:
            self.format = lib.lqreader_format(r)
            for rc in (lib.lqreader_bam_qualities(r, 1) if not self.is_sequel else 0, lib.lqreader_inflate(r, INFLATE_MODES[self.inflate]),
                       lib.lqreader_parse(r, PARSE_MODES[self.parse]), lib.lqreader_host_copy(r, HOSTCOPY_MODES[self.host_copy]),
                       lib.lqreader_bam_walk(r, BAMWALK_MODES[self.bam_walk])):
                if rc != 0:
                    raise api.LqcovError(rc, lib.lqreader_last_error(r).decode())
            chunk = ReadChunk(None, device=self.device, lib=lib)
            n, n_seqs, n_bases, last = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
            while not last.value:
                rc = lib.lqreader_next(r, chunk.h, C.byref(n), C.byref(n_seqs), C.byref(n_bases), C.byref(last))
                if rc != 0:
                    raise api.LqcovError(rc, lib.lqreader_last_error(r).decode())
                chunk._from_reader(r, n.value)
                yield chunk, n_seqs.value, n_bases.value
        finally:
            st = (C.c_uint64 * len(INFLATE_STATS))()
            if lib.lqreader_inflate_stats(r, st) == 0:
                self.inflate_stats = _stats_dict(st)
            ps = (C.c_uint64 * len(PARSE_STATS))()
            if lib.lqreader_parse_stats(r, ps) == 0:
                self.parse_stats = dict(zip(PARSE_STATS, (int(w) for w in ps)))
            cs = (C.c_uint64 * len(COPY_STATS))()
            if lib.lqreader_copy_stats(r, cs) == 0:
                self.copy_stats = dict(zip(COPY_STATS, (int(w) for w in cs)))
            lib.lqreader_close(r)
            if chunk is not None:
                chunk.close()


class FastqWriter:
    """Appends resident chunks to a FASTQ file as sampleqc.write_fastq(path, records, is_chunk=True) does (lqfastq_*): write(chunk,
    begin, end) makes the text of the chunk's reads, read i cut to [begin[i], end[i]) (None: whole reads), on the device piece by
    piece (piece_bytes, a multiple of 4096; None: the library's default) and hands the pieces to a thread that appends them to the
    file -- it returns the bytes of text, possibly before the last of them is in the file.  The file is opened (for appending) when
    the first byte comes: a writer that saw only empty chunks leaves no file.  close() waits for the thread and raises what it or
    the file reported; after an I/O or device error every later write raises it again.  A context manager."""

    def __init__(self, path, device: int = 0, piece_bytes: Optional[int] = None, lib=None):
        self.lib = _lib(lib)
        self.path, self.device, self.kernel_ms = os.fspath(path), device, 0.0
        self.h = self.lib.lqfastq_open(os.fsencode(self.path), device, int(piece_bytes or 0))
        if not self.h:
            raise api.LqcovError(-1, self.lib.lqfastq_last_error(None).decode() or "lqfastq_open failed")

    def write(self, chunk: ReadChunk, begin=None, end=None) -> int:
        if not self.h:
            raise ValueError("the writer is closed")
        begin, end = chunk.bounds_c(begin, end)
        nb, noff = chunk.names_c()
        n = C.c_uint64()
        rc = self.lib.lqfastq_write(self.h, chunk.h, nb, noff.ctypes.data, begin.ctypes.data if begin is not None else None,
                                    end.ctypes.data if end is not None else None, C.byref(n))
        if rc != 0:
            raise api.LqcovError(rc, self.lib.lqfastq_last_error(self.h).decode())
        return n.value

    def close(self):
        """the file is complete when this returns; raises the error of a piece written since the last write()"""
        if getattr(self, "h", None):
            h, self.h = self.h, None
            self.kernel_ms = float(self.lib.lqfastq_kernel_ms(h))   # k_fastq_format's time on the device, all writes (HIP events)
            rc = self.lib.lqfastq_close(h)
            if rc != 0:
                raise api.LqcovError(rc, self.lib.lqfastq_last_error(None).decode())

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                                      # (the error on its way out is the one to report)
            try:
                self.close()
            except api.LqcovError:
                pass
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _close_writers(writers, quiet: bool = False):
    """close every FastqWriter; the first error is raised when all are closed (quiet: dropped)"""
    first = None
    for w in writers:
        try:
            w.close()
        except api.LqcovError as e:
            first = first or e
    if first is not None and not quiet:
        raise first


class PackedStore:
    """The packed chunks of the whole input in device memory (lqstore_*)."""

    def __init__(self, device: int = 0, lib=None):
        self.lib = _lib(lib)
        self.h = self.lib.lqstore_create(device)
        if not self.h:
            raise api.LqcovError(-3, "lqstore_create failed (no HIP device?)")

    def append(self, chunk: ReadChunk):
        if not chunk.packed:
            chunk.pack()
        nb, noff = chunk.names_c()
        chunk._ck(self.lib.lqstore_append(self.h, chunk.h, nb, noff.ctypes.data))

    @property
    def nbytes(self) -> int:
        return int(self.lib.lqstore_bytes(self.h))

    def run(self, eng: "api.Engine"):
        eng._ck(self.lib.lqstore_run(self.h, eng.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.lqstore_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SampleQCPass:
    """The body of LongQC's chunk loop and its coverage call with every chunk uploaded once.

    add_chunk(reads) does steps 2-5 of longQC.py:305-328 on one ReadChunk: the sdust rows go to `mask` (an LqMaskMI355X: close_pool()
    writes longqc_sdust<suffix>.txt), the adapter search trims a copy of the records (kept in `trimmed`, for --trim; `adapters` is the
    AdapterStats) as the reference's pool does, the subsample (`s_reads`, seed-7 reservoir of `nsample`) and the GC fractions (`gc`, an
    LqGCMI355X) see the untrimmed reads; then the chunk is packed on the device and appended to `store`.
    coverage() maps the subsample against the stored chunks, coverage_stats() estimates the coverage from its table; figures() gives the numbers behind the GC and the length figure."""

    def __init__(self, work_dir: str, preset: str, adp5=None, adp3=None, nsample=5000, gc_draw: str = "device", device: int = 0,
                 fast: bool = False, inds: int = 4000000000, suffix: Optional[str] = None, gc_seed: int = 0, lib=None,
                 sdust_split: Optional[str] = None, sdust_table: Optional[str] = None):
        if preset not in sampleqc.PRESET_MED_SCORE:
            raise ValueError("unknown preset %r" % preset)
        self.preset, self.fast, self.inds, self.device, self.lib = preset, fast, inds, device, lib
        self.adp5, self.adp3, self.nsample = adp5, adp3, nsample
        self.mask = sdust.LqMaskMI355X(work_dir, suffix, device=device, lib=lib, split=sdust_split, table=sdust_table)     # split_mode's, table_mode's
        self.adapters = adapter.AdapterStats(adp5, adp3)
        self.gc = gcfrac.LqGCMI355X(chunk_size=150, draw=gc_draw, seed=gc_seed, device=device, lib=lib)
        self.store = PackedStore(device, lib)
        self.s_reads, self.cum_n_seq, self.chunk_n, self.n_bases = [], 0, 0, 0
        self.trimmed = None
        self.trim_writer = self.fastx_writer = None                 # FastqWriters of run_file(trim=<path>, fastx_out=<path>)

    def add_chunk(self, reads):
        chunk = ReadChunk(reads, device=self.device, lib=self.lib)
        try:
            return self._add(chunk, reads, True)
        finally:
            chunk.close()

    def add_resident(self, chunk: ReadChunk, trim=False):
        """add_chunk on a chunk that is on the device already (FileChunks'): nothing is gathered or uploaded, and of the reads only
        the subsample's winners come to the host -- with trim=True (--trim) all of them, for `trimmed`.  trim=<a FastqWriter>: the
        trimmed reads go to it from the device (k_fastq_format), `trimmed` stays None and no further read comes to the host"""
        return self._add(chunk, None, trim)

    def _add(self, chunk, reads, trim):
        self.mask.submit_sdust(reads, self.chunk_n, chunk=chunk)                                        # longQC.py:307
        result = None
        writer = trim if isinstance(trim, FastqWriter) else None
        if self.adp5 or self.adp3:                                                                      # :310-320, on a copy as the pool's pickling makes one
            self.trimmed = ([list(r) for r in reads] if reads is not None else chunk.records()) if trim and not writer else None
            bounds = [] if writer else None
            result = adapter.cut_adapter(self.trimmed, adp_t=self.adp5, adp_b=self.adp3, chunk=chunk, bounds_out=bounds)
            self.adapters.add(result)                                                                   # :348-357
            if writer:
                writer.write(chunk, *bounds)                                                            # :345-346
        if reads is not None:
            self.s_reads = sampleqc.subsample_from_chunk(reads, self.cum_n_seq, self.s_reads, self.nsample)    # :323
        else:
            self.s_reads = sampleqc.subsample_from_resident(chunk, self.cum_n_seq, self.s_reads, self.nsample)
        self.gc.calc_read_and_chunk_gc_frac(reads, chunk=chunk)                                         # :328
        self.store.append(chunk)
        self.chunk_n += 1
        self.cum_n_seq += chunk.n
        self.n_bases += int(chunk.lens.sum())
        return result

    def run_file(self, path: str, chunk_size=0.5 * 1024 ** 3, trim=False, is_upper: bool = True, str_overhead: Optional[int] = None,
                 is_sequel: bool = True, inflate: Optional[str] = None, fastx_out=None, parse: Optional[str] = None,
                 host_copy: Optional[str] = None, sdust_split: Optional[str] = None, bam_walk: Optional[str] = None,
                 sdust_table: Optional[str] = None):
        """the whole loop of longQC.py:299-360 over a plain or gzip FASTA/FASTQ file or an unaligned BAM (is_sequel, inflate, parse,
        host_copy, bam_walk: FileChunks'): FileChunks + add_resident.  -> the per-chunk adapter results; with trim=True `trimmed_chunks` holds every chunk's
        trimmed records (longQC.py:330-338 writes them out).  trim=<path> (str or os.PathLike): every chunk's trimmed reads are
        appended to that file from the device (a FastqWriter; the file write_fastq(path, trimmed, is_chunk=True) per chunk makes),
        `trimmed` stays None and `trimmed_chunks` empty.  fastx_out=<path>: every chunk is appended to that file untrimmed -- the
        FASTQ that longQC.py:302-303 converts a BAM file to, for any input.  Both files are complete, and their errors raised, when
        the call returns.  sdust_split: split_mode's, for this file (None: what the constructor was given); the table is the same.
        sdust_table: sdust.table_mode's, for this file in the same way ("device": the rows are formatted on the device)."""
        mask_split, mask_table = self.mask.split, self.mask.table
        if sdust_split is not None:
            self.mask.split = split_mode(sdust_split)
        if sdust_table is not None:
            self.mask.table = sdust.table_mode(sdust_table)
        results, self.trimmed_chunks = [], []
        to_file = isinstance(trim, (str, os.PathLike))
        if to_file and not (self.adp5 or self.adp3):
            raise ValueError("trim=<path> needs an adapter")
        writers = []
        try:
            if to_file:
                self.trim_writer = trim = FastqWriter(trim, device=self.device, lib=self.lib)
                writers.append(trim)
            if fastx_out is not None:
                self.fastx_writer = FastqWriter(fastx_out, device=self.device, lib=self.lib)
                writers.append(self.fastx_writer)
            for chunk, _n_seqs, _n_bases in FileChunks(path, chunk_size, is_upper, self.device, str_overhead, lib=self.lib, is_sequel=is_sequel,
                                                        inflate=inflate, parse=parse, host_copy=host_copy, bam_walk=bam_walk):
                if fastx_out is not None:
                    self.fastx_writer.write(chunk)                                                      # longQC.py:302-303
                results.append(self.add_resident(chunk, trim=trim))
                if trim and not isinstance(trim, FastqWriter):
                    self.trimmed_chunks.append(self.trimmed)
        except BaseException:
            _close_writers(writers, quiet=True)                    # (the loop's error is the one to report)
            raise
        finally:
            self.mask.split, self.mask.table = mask_split, mask_table      # (sdust_split and sdust_table held for this file)
        _close_writers(writers)
        return results

    def coverage(self, s_reads=None, short_threshold: Optional[int] = None, out: Optional[str] = None, exclude_seqs=None, chunks=None):
        """The coverage table of the subsample (s_reads: another query set) against every chunk added, as
        sampleqc.coverage_in_memory(chunks, s_reads, preset, ...) gives it: the text, or with short_threshold (LongQC's --short) the
        (main, short) pair mapped in one pass; `out` gets the text (the pair: concatenated).  exclude_seqs (with `chunks`, the re-iterable
        input): sampleqc.replace_masked first, longQC.py:369-406 -- the one step that reads the input again, as the reference does."""
        reads = self.s_reads if s_reads is None else s_reads
        if exclude_seqs:
            reads = sampleqc.replace_masked(reads, exclude_seqs, chunks if chunks is not None else [])
        inds = str(self.inds)
        if short_threshold is None:
            text = self._pass([(reads, sampleqc.coverage_argv(self.preset, "-", "-", fast=self.fast, inds=inds))])[0]
        else:
            main_reads, short_reads = sampleqc.short_split(reads, short_threshold)
            argv_main = sampleqc.coverage_argv(self.preset, "-", "-", fast=self.fast, inds=inds)
            argv_short = sampleqc.coverage_argv(self.preset, "-", "-", fast=self.fast, inds=inds, short=True)
            strip_p = lambda a: [x for i, x in enumerate(a) if x != "-p" and (i == 0 or a[i - 1] != "-p")]
            if strip_p(argv_main) == strip_p(argv_short):
                text = tuple(self._pass([(main_reads, argv_main), (short_reads, argv_short)]))
            else:                                                  # other index options: a pass of its own over the same stored chunks
                text = (self._pass([(main_reads, argv_main)])[0], self._pass([(short_reads, argv_short)])[0])
        self.table_text = text if isinstance(text, str) else "".join(text)       # (for coverage_stats)
        if out:
            with open(out, "w") as f:
                f.write(self.table_text)
        return text

    def coverage_stats(self, is_transcript=False):
        """The Coverage_stats entries of the run's JSON (longQC.py:659-681) from the table coverage() made last (with short_threshold: the
        pair concatenated, LongQC's merged table): covtable.CoverageTable(table).est_coverage(is_transcript).json_block(throughput) with
        both mixture fits on the device (mixfit) and the bases of every chunk added as the throughput (longQC.py:468).  `coverage_table`
        keeps the CoverageTable for the getters and the figure data"""
        from . import covtable
        if getattr(self, "table_text", None) is None:
            raise RuntimeError("coverage_stats() reads the table of coverage(): call that first")
        self.coverage_table = covtable.CoverageTable(io.StringIO(self.table_text))
        self.coverage_table.est_coverage(is_transcript, device=self.device, lib=self.lib)
        return self.coverage_table.json_block(self.n_bases)

    def _pass(self, sets):
        """one run over the stored chunks for every (reads, argv) of `sets` -> one table per set"""
        p, _, _ = api.parse_args(sets[0][1])
        eng = api.Engine(p, device=self.device, lib=self.lib)
        try:
            sampleqc.set_query_reads(eng, sets)
            self.store.run(eng)
            eng.finish()
            return [eng.table_text()] if len(sets) == 1 else [eng.table_text(set=k) for k in range(len(sets))]
        finally:
            eng.close()

    def summary(self):
        """the mask's summary (LqMaskMI355X.summary): what longQC.py:369-371, 452-471 read back from the table"""
        return self.mask.summary()

    def figures(self, per_read=False):
        """the numbers behind the GC figure and the length figure of every chunk added (LqGCMI355X.figure_data,
        LqMaskMI355X.length_figure_data): what longQC.py:449,487-488 compute before they draw.  per_read: also "qscore" and "masked", the
        QV box plot by length bin and the masked-fraction histogram of lq_mask.py:43-79 (qscore_figure_data, masked_fraction_data)"""
        out = {"gc": self.gc.figure_data(), "length": self.mask.length_figure_data()}
        if per_read:
            out["qscore"], out["masked"] = self.mask.qscore_figure_data(), self.mask.masked_fraction_data()
        return out

    def close(self):
        self.store.close()

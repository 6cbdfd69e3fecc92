"""Host side of the low-complexity table: the counterpart of lq_mask.py's use of the
reference's `sdust` binary (lq_mask.py:17-23 `_sdust`, :99-121 `submit_sdust` / `close_pool`), over the C ABI of
include/lqcov.h (lqsdust_main, lqsdust_reads).  No CPU fallback: without liblqcov.so or a HIP device the calls raise."""
import ctypes as C
import math
import os
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

from . import api


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqsdust_bound", False):
        lib.lqsdust_main.restype = C.c_int
        lib.lqsdust_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, C.c_int]
        lib.lqsdust_reads.restype = C.c_int
        lib.lqsdust_reads.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lqsdust_format.restype = C.c_int
        lib.lqsdust_format.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lqsdust_format_lists.restype = C.c_int
        lib.lqsdust_format_lists.argtypes = lib.lqsdust_format.argtypes[:-2] + [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        lib.lqsdust_fmt3.restype = C.c_uint32
        lib.lqsdust_fmt3.argtypes = [C.c_double, C.c_void_p]
        lib._lqsdust_bound = True
    return lib


SPLIT_MODES = ("serial", "pieces")
SPLIT_PIECE = 4096                                         # LQ_DUST_SPLIT_PIECE: bases per piece unless the caller says otherwise
SPLIT_MIN_PIECES = 2                                       # LQ_DUST_SPLIT_MIN_PIECES: a read of fewer pieces' bases takes the serial walk


def split_mode(split):
    """"serial" | "pieces" | None (the environment variable LQSDUST_SPLIT, "serial" without it) -> the mode's name.  "pieces": reads
    of A/C/G/T alone with two pieces' bases or more are cut into pieces scanned side by side (k_sdust_pieces); the table is the same"""
    mode = os.environ.get("LQSDUST_SPLIT", "serial") if split is None else split
    if mode not in SPLIT_MODES:
        raise ValueError("split must be 'serial' or 'pieces', not %r" % (mode,))
    return mode


TABLE_MODES = ("host", "device")
TABLE_STATS = ("rows", "bytes", "masked", "q7", "unvouched", "excluded", "excluded_first", "reserved")      # lqsdust_stats' words
ROW_FIELDS_MAX = 48                                        # a row's bytes beside its name at most: lqchunk_sdust_table's capacity rule


def table_mode(table):
    """"host" | "device" | None (the environment variable LQSDUST_TABLE, "host" without it) -> the mode's name.  "device": the rows of a
    resident chunk are formatted on the device (k_sdust_rows, k_sdust_text) and leave it as bytes; the table is the same"""
    mode = os.environ.get("LQSDUST_TABLE", "host") if table is None else table
    if mode not in TABLE_MODES:
        raise ValueError("table must be 'host' or 'device', not %r" % (mode,))
    return mode


def stats_dict(words):
    d = dict(zip(TABLE_STATS, (int(w) for w in words)))
    del d["reserved"]
    return d


def with_lists(stats, excl):
    """stats and the index array lqchunk_sdust_table / lqsdust_format_lists filled -> stats with exclude_first and exclude_second"""
    k1, k = stats["excluded_first"], stats["excluded"]
    stats["exclude_first"], stats["exclude_second"] = excl[:k1].tolist(), excl[k1:k].tolist()
    return stats


def fmt3(x: float, lib=None):
    """"%.3f" of x as the table's kernels take it (lqsdust_fmt3): -> (class: 0 finite, 1 nan, 2 inf, 3 2^50 or more, + 4 with the sign
    bit; thousandths of |x|)"""
    t = C.c_uint64()
    return int(_lib(lib).lqsdust_fmt3(float(x), C.byref(t))), t.value


def format_rows(names: Sequence[str], masked, lens, psum, has_q, qv, window: float = 0.0, device: int = 0, lib=None, out_cap: Optional[int] = None):
    """Arrays -> the table's text, made on the device (lqsdust_format): row i is what _rows prints for masked[i], lens[i], psum[i], qv[i]
    and -- has_q[i] != 0 and lens[i] > 0 -- qualities.  window: 0 the default (2^-30), 1 every row with qualities takes the host's
    meanQ.  -> (bytes, stats: a dict of TABLE_STATS and, as ReadChunk.sdust_table's, exclude_first / exclude_second, the ascending indices
    of the rows on LongQC's two exclusion lists: lqsdust_format_lists)"""
    lib = _lib(lib)
    n = len(names)
    nb, noff = api.encode_names(list(names))
    masked, lens, qv = (np.ascontiguousarray(a, dtype=np.uint32) for a in (masked, lens, qv))
    psum = np.ascontiguousarray(psum, dtype=np.float64)
    has_q = np.ascontiguousarray(has_q, dtype=np.uint8) if has_q is not None else None
    if any(a.shape != (n,) for a in (masked, lens, qv, psum)) or (has_q is not None and has_q.shape != (n,)):
        raise ValueError("one entry per name in every array")
    cap = len(nb) - n + ROW_FIELDS_MAX * n if out_cap is None else int(out_cap)
    out, n_out, st, err = np.empty(max(cap, 1), np.uint8), C.c_uint64(), (C.c_uint64 * len(TABLE_STATS))(), C.create_string_buffer(512)
    excl = np.zeros(max(2 * n, 1), np.uint32)
    rc = lib.lqsdust_format_lists(device, n, nb, noff.ctypes.data, masked.ctypes.data, lens.ctypes.data, psum.ctypes.data,
                                  has_q.ctypes.data if has_q is not None else None, qv.ctypes.data, float(window), out.ctypes.data, cap, C.byref(n_out), st,
                                  excl.ctypes.data, 2 * n, err, 512)
    if rc != 0:
        raise api.LqcovError(rc, err.value.decode())
    return out[:n_out.value].tobytes(), with_lists(stats_dict(st), excl)


def run_sdust(fin: str, fout: str, device: int = 0, w: Optional[int] = None, t: Optional[int] = None, lib=None) -> None:
    """== lq_mask._sdust(psdust, fin, fout): `sdust <fin>` with stdout -> fout (lq_mask.py:17-23)"""
    lib = _lib(lib)
    argv = [b"sdust"]
    if w is not None:
        argv += [b"-w", str(w).encode()]
    if t is not None:
        argv += [b"-t", str(t).encode()]
    argv.append(fin.encode())
    arr = (C.c_char_p * len(argv))(*argv)
    err = fout + ".stderr"
    rc = lib.lqsdust_main(len(argv), arr, fout.encode(), err.encode(), device)
    msg = open(err).read() if os.path.exists(err) else ""
    if os.path.exists(err):
        os.remove(err)
    if rc == 0 and msg and os.environ.get("LQCOV_TIMING"):
        import sys
        sys.stderr.write(msg)
    if rc != 0:
        raise api.LqcovError(rc if rc < 0 else -2, msg.strip() or "sdust failed")


def sdust_rows(names: Sequence[str], seqs: Sequence[np.ndarray], quals: Optional[Sequence[Optional[np.ndarray]]] = None,
               device: int = 0, w: int = 64, t: int = 20, lib=None, chunk=None, split: Optional[str] = None,
               piece: Optional[int] = None) -> List[str]:
    """Reads in memory (no temporary FASTQ as in lq_mask.py:108-114) -> the rows `sdust` would print for them.
    chunk: a chunkpass.ReadChunk that holds these reads on the device already -- seqs and quals are not looked at, nothing is
    gathered or uploaded.  split, piece: split_mode's; "pieces" scans long reads in pieces of `piece` bases (lqchunk_sdust_split) --
    the rows are the same."""
    return _rows(names, *_scan(names, seqs, quals, device, w, t, lib, chunk, split, piece))


def _scan(names, seqs, quals, device, w, t, lib, chunk, split, piece):
    """sdust_rows' scan -> (n, off, qflat, masked, psum, qv), what _rows takes behind the names"""
    split = split_mode(split)
    if chunk is not None:
        return (chunk.n, chunk.off, chunk.qual_first()) + tuple(chunk.sdust(w, t, split=split, piece=piece))
    if split == "pieces":                                  # (the pieces live on a resident chunk: one for this call)
        ch = _chunk_of(names, seqs, quals, device, lib)
        try:
            return (ch.n, ch.off, ch.qual_first()) + tuple(ch.sdust(w, t, split=split, piece=piece))
        finally:
            ch.close()
    lib = _lib(lib)
    n = len(seqs)
    off = np.zeros(n + 1, dtype=np.uint64)
    for i, s in enumerate(seqs):
        off[i + 1] = off[i] + s.shape[0]
    flat = np.concatenate([np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]) if n else np.zeros(0, np.uint8)
    qflat = None
    if quals is not None and any(q is not None and q.shape[0] for q in quals):
        qflat = np.zeros(int(off[n]), dtype=np.uint8)
        for i, q in enumerate(quals):
            if q is not None and q.shape[0]:
                qflat[int(off[i]):int(off[i + 1])] = q
    masked = np.zeros(max(n, 1), dtype=np.uint32)
    psum = np.zeros(max(n, 1), dtype=np.float64)
    qv = np.zeros(max(n, 1), dtype=np.uint32)
    err = C.create_string_buffer(512)
    rc = lib.lqsdust_reads(device, n, flat.ctypes.data if n else None, off.ctypes.data, qflat.ctypes.data if qflat is not None else None,
                           w, t, masked.ctypes.data, psum.ctypes.data, qv.ctypes.data, err, 512)
    if rc != 0:
        raise api.LqcovError(rc, err.value.decode())
    return n, off, qflat, masked, psum, qv


def _chunk_of(names, seqs, quals, device, lib):
    """a resident chunk of reads in memory, for one call"""
    from . import chunkpass
    qs = quals if quals is not None else [None] * len(seqs)
    reads = [[nm, bytes(s), bytes(q) if q is not None and q.shape[0] else None] for nm, s, q in zip(names, seqs, qs)]
    return chunkpass.ReadChunk(reads, device=device, lib=lib)


def _rows(names, n, off, qflat, masked, psum, qv) -> List[str]:
    """qflat: the qualities on the host (None: none), or True: every read with bases has qualities (a chunk read from a file)"""
    rows = []
    for i in range(n):
        ln = int(off[i + 1] - off[i])
        has_q = ln > 0 and (qflat is True or (qflat is not None and qflat[int(off[i])] != 0))
        frac = _c_div(float(masked[i]), ln)
        mq = -10 * _c_log10(_c_div(float(psum[i]) if has_q else 0.0, ln if has_q else 0))
        rows.append("%s\t%d\t%d\t%s\t%s\t%d" % (names[i], int(masked[i]), ln, _c_fmt3(frac), _c_fmt3(mq), int(qv[i])))
    return rows


class LqMaskMI355X:
    """Counterpart of lq_mask.LqMask for the chunk loop of longQC.py (lq_mask.py:25-41, 99-121): submit_sdust(reads,
    chunk_n) per chunk, close_pool() at the end, get_outfile_path() -> analysis table `longqc_sdust<suffix>.txt` with one
    row per read in submission order.  Reads are LongQC's [name, seq, qual, ...] records (str or bytes); no temporary
    FASTQ files, no process pool: every chunk is one call into the device.  Nothing is plotted: length_figure_data() gives the numbers of
    the length figure (histogram, gamma fit), masked_fraction_data() and qscore_figure_data() those of the masked-fraction histogram and of
    the QV box plot by length bin (lq_mask.py:43-79), from the two "%.3f" columns kept per chunk as the thousandths the file shows.
    table (table_mode's) "device": a chunk's rows are formatted on the device and kept as bytes (ReadChunk.sdust_table); the file is the
    same.  summary() and json_block() give what longQC.py:369-371, 452-471, 495-502 read back from the file, from arrays kept at submit
    time in either mode."""

    def __init__(self, work_dir: str, suffix: Optional[str] = None, device: int = 0, lib=None, split: Optional[str] = None,
                 table: Optional[str] = None):
        self.split = split_mode(split)                         # "pieces": long reads are scanned in pieces, the rows are the same
        self.table = table_mode(table)                         # "device": the rows are formatted there, the file is the same
        self.suffix = "_" + suffix if suffix else ""
        os.makedirs(work_dir, exist_ok=True)
        self.wdir, self.device, self.lib = work_dir, device, lib
        self.outf = os.path.join(work_dir, "longqc_sdust" + self.suffix + ".txt")
        self._chunks = {}
        self._lens, self._excl = {}, {}                        # per chunk: the lengths; the names on the two exclusion lists
        self._cols = {}                                        # per chunk: the printed fraction and meanQ as thousandths (columns_of_rows)
        self._masked = self._q7 = 0

    @staticmethod
    def _arr(v):
        if v is None:
            return None
        if isinstance(v, str):
            v = v.encode()
        return np.frombuffer(bytes(v), dtype=np.uint8)

    def submit_sdust(self, reads, chunk_n, chunk=None):
        """chunk: the chunkpass.ReadChunk made of `reads` (its device copy is scanned; `reads` is not gathered again)"""
        if self.table == "device":
            own = chunk is None
            if own:                                            # (the table is made from a resident chunk: one for this call)
                names = [r[0].decode() if isinstance(r[0], (bytes, bytearray)) else str(r[0]) for r in reads]
                chunk = _chunk_of(names, [self._arr(r[1]) for r in reads], [self._arr(r[2]) if len(r) > 2 and r[2] else None for r in reads],
                                  self.device, self.lib)
            try:
                text, st = chunk.sdust_table(split=self.split)
                self._chunks[chunk_n] = text
                self._note(chunk_n, chunk.lens, st["masked"], st["q7"], [chunk.names[i] for i in st["exclude_first"]],
                           [chunk.names[i] for i in st["exclude_second"]], *chunk.sdust_columns())
            finally:
                if own:
                    chunk.close()
            return
        if chunk is not None:
            names, seqs, quals = chunk.names, None, None
        else:
            names = [r[0].decode() if isinstance(r[0], (bytes, bytearray)) else str(r[0]) for r in reads]
            seqs = [self._arr(r[1]) for r in reads]
            quals = [self._arr(r[2]) if len(r) > 2 and r[2] else None for r in reads]
        n, off, qflat, masked, psum, qv = _scan(names, seqs, quals, self.device, 64, 20, self.lib, chunk, self.split, None)
        self._chunks[chunk_n] = _rows(names, n, off, qflat, masked, psum, qv)
        lens = np.diff(np.asarray(off).astype(np.int64))
        first, second = exclusion_lists(masked[:n], lens)
        self._note(chunk_n, lens, int(masked[:n].sum(dtype=np.uint64)), int(qv[:n].sum(dtype=np.uint64)), [names[i] for i in first], [names[i] for i in second],
                   *columns_of_rows(self._chunks[chunk_n]))

    def _note(self, chunk_n, lens, masked, q7, first, second, frac_thou=None, qv_thou=None):
        """frac_thou, qv_thou: the chunk's two printed columns; None: not kept, every read counts as "-nan" in the per-read figures"""
        self._lens[chunk_n] = np.array(lens, dtype=np.int64)
        n = self._lens[chunk_n].shape[0]
        self._cols[chunk_n] = (np.array(frac_thou, dtype=np.uint32) if frac_thou is not None else np.full(n, 0xffffffff, np.uint32),
                               np.array(qv_thou, dtype=np.int32) if qv_thou is not None else np.full(n, -2 ** 31, np.int32))
        self._excl[chunk_n] = (first, second)
        self._masked += int(masked)
        self._q7 += int(q7)

    def close_pool(self):
        with open(self.outf, "w") as out:                      # lq_mask.py:83-88 concatenates the chunk tables in submission order
            for k in self._chunks:
                if isinstance(self._chunks[k], bytes):             # (a chunk's table from the device)
                    out.flush()
                    out.buffer.write(self._chunks[k])
                    continue
                for row in self._chunks[k]:
                    out.write(row + "\n")
        self._chunks = {}

    def get_outfile_path(self):
        return self.outf

    def summary(self):
        """What longQC.py reads back from the table (:369-371, 452-471), from the arrays kept at submit time, every chunk submitted so far:
        n_reads, yield, longest, mean_length, n50 (lq_utils.get_N50: the first of the descending lengths at which the running sum reaches
        half the yield), q7_bases, masked_bases, and exclude_seqs: the names of the reads with len > 500000 and a printed fraction above
        0.2, then of those with len > 10000 and above 0.4, each list in file order (a read on both is named twice).  No reads: 0 everywhere"""
        lens = np.concatenate([self._lens[k] for k in self._lens]) if self._lens else np.zeros(0, np.int64)
        n, total = int(lens.shape[0]), int(lens.sum())
        n50 = 0
        if n:
            d = np.sort(lens)[::-1]
            n50 = int(d[int(np.searchsorted(np.cumsum(d), total / 2, side="left"))])
        excl = [nm for which in (0, 1) for k in self._excl for nm in self._excl[k][which]]
        return {"n_reads": n, "yield": total, "longest": int(lens.max()) if n else 0, "mean_length": float(lens.mean()) if n else 0.0, "n50": n50,
                "q7_bases": self._q7, "masked_bases": self._masked, "exclude_seqs": excl}

    def length_figure_data(self, b_width=1000) -> dict:
        """What longQC.py:487-488 computes for the length figure, on the device (figdata.py), every chunk submitted so far: hist = (edges,
        counts, density) of plt.hist(lengths, bins=np.arange(min(lengths), longest + b_width, b_width), density=True) (lq_gamma.py:54),
        gamma_params = (a, scale) of gamma.fit(lengths, floc=0.0) (lq_gamma.py:47-49), and mean_length, n50, longest of summary().
        ValueError for no reads, for a read of length 0 (scipy's FitDataError is one), and for lengths without spread (one read, or all
        equal: log(mean) - mean(log) is not above the rounding of its two sums, and no shape maximises the likelihood)"""
        from . import figdata
        lens = np.concatenate([self._lens[k] for k in self._lens]) if self._lens else np.zeros(0, np.int64)
        n = int(lens.shape[0])
        if n == 0:
            raise ValueError("no reads submitted")
        if int(lens.max()) >= 1 << 32:
            raise ValueError("a read of 2^32 bases or more")
        u = lens.astype(np.uint32)
        total, sum_log, zeros = figdata.log_sums(u, self.device, self.lib)
        if zeros:
            raise ValueError("Invalid values in `data`.  Maximum likelihood estimation with 'gamma' requires that 0 < x < inf for each x in `data`.")
        # the rounding of s = log(mean) - sum_log / n: a unit each for the logarithm and the two divisions, and the device sum's bound
        # (a logarithm, 256 sequential additions and a tree of log2 n levels, on non-negative terms)
        s_err = (3 * abs(math.log(total / n)) + (2 + 256 + math.log2(n)) * abs(sum_log / n)) * 2.0 ** -53
        if not math.log(total / n) - sum_log / n > s_err:
            raise ValueError("the lengths have no spread that their sums can show: no gamma shape maximises the likelihood")
        s = self.summary()
        lo, _ = figdata.value_range(u, self.device, self.lib)
        return {"hist": figdata.density_hist(u, int(lo), s["longest"] + b_width, b_width, self.device, self.lib),
                "gamma_params": figdata.gamma_fit(n, total, sum_log), "mean_length": s["mean_length"], "n50": s["n50"], "longest": s["longest"]}

    def columns(self):
        """-> (lengths int64, printed fractions as uint32 thousandths, printed meanQ as int32 thousandths) of every chunk submitted so far,
        in file order: what pandas reads from columns 2, 3 and 4 of the file, times 1000; "-nan" is 0xffffffff / figdata.MISSING"""
        if not self._lens:
            return np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.int32)
        return (np.concatenate([self._lens[k] for k in self._lens]), np.concatenate([self._cols[k][0] for k in self._cols]),
                np.concatenate([self._cols[k][1] for k in self._cols]))

    def qscore_figure_data(self, interval=None, platform="ont") -> dict:
        """What lq_mask.py:43-68 computes for the QV box plot by length bin, on the device (figdata.box_stats), every chunk submitted so
        far: the reads are binned by np.floor(length / interval), interval 3000 or n50 / 2 where n50 < 3000 (longQC.py:478-481) unless the
        caller names one, and each bin's printed meanQ values get matplotlib's box (whis 1.5; a read without qualities is left out, as pandas
        drops its NaN).  -> box_stats' dict and "interval", "mid_threshold" (7 for ont, else 8: lq_mask.py:44-47).  ValueError for no reads"""
        from . import figdata
        lens, _, qv = self.columns()
        if lens.shape[0] == 0:
            raise ValueError("no reads submitted")
        if int(lens.max()) >= 1 << 32:
            raise ValueError("a read of 2^32 bases or more")
        if interval is None:
            n50 = self.summary()["n50"]
            interval = 3000 if n50 >= 3000 else n50 / 2
        if not interval > 0:
            raise ValueError("the length interval must be positive, not %r" % (interval,))
        out = figdata.box_stats(lens.astype(np.uint32), qv, float(interval), 1.5, self.device, self.lib)
        out["interval"], out["mid_threshold"] = interval, 7 if platform == "ont" else 8
        return out

    def masked_fraction_data(self):
        """What lq_mask.py:70 computes for the masked-fraction figure, on the device: (edges, counts) of np.histogram(fractions,
        bins=np.arange(0, 1.0, 0.01)) on the printed fractions of every chunk submitted so far (figdata.masked_fraction_hist).  A read of
        length 0 ("-nan") and a fraction printed above 0.990 are counted nowhere, as there.  ValueError for no reads"""
        from . import figdata
        _, frac, _ = self.columns()
        if frac.shape[0] == 0:
            raise ValueError("no reads submitted")
        return figdata.masked_fraction_hist(frac, self.device, self.lib)

    def json_block(self, with_gamma=False):
        """the entries of longQC.py:495-502 that come from the table; with_gamma: Length_stats also holds "gamma_params": [a, scale], the
        fit of longQC.py:487,500 (length_figure_data, figdata.gamma_fit), in the reference's place"""
        s = self.summary()
        if not s["n_reads"] or not s["yield"]:
            raise ValueError("no bases submitted")
        stats = {"Mean_read_length": s["mean_length"], "N50_read_length": float(s["n50"])}
        if with_gamma:
            a, scale = self.length_figure_data()["gamma_params"]
            stats = {"gamma_params": [float(a), float(scale)], **stats}
        return {"Yield": s["yield"], "Q7 bases": "%.2f%%" % float(100 * s["q7_bases"] / s["yield"]), "Longest_read": s["longest"],
                "Num_of_reads": s["n_reads"], "Length_stats": stats}


def thou_of_text(t: str):
    """a "%.3f" field -> its thousandths as an int ("-0.000" is 0), None for "-nan" / "nan"; an infinite value raises ValueError"""
    if t.endswith("nan"):
        return None
    if t[-4:-3] != ".":
        raise ValueError("not a %%.3f number: %r" % (t,))
    return int(t[:-4] + t[-3:])


def columns_of_rows(rows):
    """the table's rows (sdust._rows') -> (fractions uint32, meanQ int32): the thousandths their two "%.3f" fields show; "-nan" is
    0xffffffff / figdata.MISSING -- lqchunk_sdust_columns' arrays"""
    frac, qv = np.zeros(len(rows), np.uint32), np.zeros(len(rows), np.int32)
    for i, row in enumerate(rows):
        f, q = (thou_of_text(t) for t in row.rsplit("\t", 3)[1:3])
        frac[i] = 0xffffffff if f is None else f
        qv[i] = -2 ** 31 if q is None else q
    return frac, qv


def _printed_above(thou: int) -> float:
    """the smallest double that "%.3f" prints above thou / 1000: printf rounds the binary value exactly, so x prints above it exactly when
    x > (thou + 0.5) / 1000 -- no double is that border (2000 has the factor 125), so no tie exists -- and one comparison decides"""
    border = Fraction(2 * thou + 1, 2000)
    c = float(border)                                      # (the nearest double, on either side)
    return c if Fraction(c) > border else math.nextafter(c, math.inf)


_ABOVE_200, _ABOVE_400 = _printed_above(200), _printed_above(400)


def exclusion_lists(masked, lens):
    """longQC.py:370-371 on arrays: the reads with len > 500000 and masked/len printed above 0.200, and those with len > 10000 and
    printed above 0.400 -- pandas compares what it parsed, the "%.3f" text -> two ascending index lists.  Array work alone: the double
    masked / len (the division _rows prints) against the smallest double that prints above the threshold"""
    masked, lens = np.asarray(masked).astype(np.float64), np.asarray(lens).astype(np.int64)
    frac = masked / np.maximum(lens, 1)
    first = np.flatnonzero((lens > 500000) & (frac >= _ABOVE_200))
    second = np.flatnonzero((lens > 10000) & (frac >= _ABOVE_400))
    return first.tolist(), second.tolist()


def _c_div(a: float, b: int) -> float:
    return a / b if b else math.nan                       # C: 0.0 / 0 (x86: the default NaN, printed "-nan")


def _c_log10(x: float) -> float:
    if x != x:
        return x
    return math.log10(x) if x > 0 else (-math.inf if x == 0 else math.nan)


def _c_fmt3(x: float) -> str:
    if x != x:
        return "-nan"                                     # x86 keeps the sign of the default NaN through log10 and the product
    if x in (math.inf, -math.inf):
        return "inf" if x > 0 else "-inf"
    return "%.3f" % x

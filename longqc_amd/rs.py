"""LongQC's `runqc -p rs` on the device: what lq_rs.run_platformqc (lq_rs.py:93-222) computes from the *.sts.csv and *.sts.xml of an RS-II
run -- the HQ-region lengths of the ZMWs with ReadScore > 0.1, their sum, maximum, mean, N50 / N90 and gamma fit, the HQ fraction, the
two length histograms and the ReadScore box plot by length bin -- without pandas, scipy or matplotlib.  The table is read into typed
columns on the device (kernels_csv.hpp behind lqcsv_* of include/lqcov.h) and the statistics run on the columns where they lie; the host
reads the header line, the sts.xml and a few numbers.  Nothing is drawn: run_platformqc returns what the two figures plot.  No CPU
fallback: without liblqcov.so or a HIP device the calls raise.

    js, fig = run_platformqc(run_dir, out_dir)        # out_dir/QC_vals_rs.json is written; js is its content

The table's domain: comma-separated, one header line, no quotes, every row with the header's field count, plain
numbers in the wanted columns.  Anything else raises LqcovError with the line and the reason.  Not built: quoted fields, NA values, an
implicit index column, ragged rows, other separators.  A caller who wants the columns themselves uses StsTable."""
import ctypes as C
import json
import os
import xml.etree.ElementTree as et

import numpy as np

from . import api, figdata

INT64, DOUBLE = 0, 1                                               # LQCSV_INT64 / LQCSV_DOUBLE
HQ, BASES, LEN_ALL = 0, 1, 2                                       # LQCSV_HQ / LQCSV_BASES / LQCSV_LEN_ALL
STATS = ("rows", "fields_device", "fields_host", "pieces", "bytes")
LENGTHS = ("n", "sum_hq", "min_hq", "max_hq", "n50", "n90", "sum_bases", "min_bases", "max_bases", "reserved")
COLUMNS = (("ReadScore", DOUBLE), ("HQRegionStart", INT64), ("HQRegionEnd", INT64), ("NumBases", INT64))
STS_NS = "http://pacificbiosciences.com/PipelineStats/PipeStats.xsd"
# lqfig_box_f64 of include/lqcov.h
BOX = np.dtype([("group", np.uint32), ("reserved", np.uint32), ("first", np.uint64), ("n_all", np.uint64), ("n", np.uint64),
                ("mid_lo", np.float64), ("mid_hi", np.float64), ("q1", np.float64), ("med", np.float64), ("q3", np.float64),
                ("whislo", np.float64), ("whishi", np.float64), ("n_low", np.uint64), ("n_high", np.uint64)])
assert BOX.itemsize == 104
BOX_CAP_FIRST = 65536


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqcsv_bound", False):
        H, v, u64, u32, dbl = C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double
        lib.lqcsv_create.restype, lib.lqcsv_create.argtypes = H, [C.c_int]
        lib.lqcsv_destroy.restype, lib.lqcsv_destroy.argtypes = None, [H]
        lib.lqcsv_last_error.restype, lib.lqcsv_last_error.argtypes = C.c_char_p, [H]
        for name, args in (("lqcsv_want", [H, C.c_char_p, C.c_int]), ("lqcsv_set_piece_bytes", [H, u64]), ("lqcsv_add_bytes", [H, v, u64, C.c_int, v]),
                           ("lqcsv_add_file", [H, C.c_char_p]), ("lqcsv_finish", [H, v]), ("lqcsv_get", [H, u32, v]), ("lqcsv_stats", [H, v]),
                           ("lqcsv_lengths", [H, u32, dbl, u32, u32, u32, v]), ("lqcsv_get_lengths", [H, C.c_int, v]),
                           ("lqcsv_hist", [H, C.c_int, v, u32, v]), ("lqcsv_logsum", [H, v, v, v]), ("lqcsv_boxstats", [H, u32, dbl, dbl, v, v, u32, v]),
                           ("lqfig_boxstats_f64", [C.c_int, v, v, u64, dbl, dbl, v, v, u32, v, C.c_char_p, C.c_size_t])):
            f = getattr(lib, name)
            f.restype, f.argtypes = C.c_int, args
        lib._lqcsv_bound = True
    return lib


def _ptr(a):
    return a.ctypes.data if a.size else None


# ---- box-plot statistics of doubles by group --------------------------------------------------------------------------------------------
def _box_dict(s, b):
    out = {f: b[f].copy() for f in ("group", "n", "q1", "med", "q3", "whislo", "whishi")}
    out["median"] = (b["mid_lo"] + b["mid_hi"]) / 2                 # np.median's and pandas': the mean of the two middle values
    out["fliers"] = [np.concatenate([s[f:f + lo], s[f + n - hi:f + n]])
                     for f, n, lo, hi in zip(b["first"].astype(np.int64).tolist(), b["n"].astype(np.int64).tolist(), b["n_low"].astype(np.int64).tolist(), b["n_high"].astype(np.int64).tolist())]
    return out


def box_stats_f64_raw(key, x, interval: float = 0.0, whis: float = 1.5, device: int = 0, lib=None):
    """lqfig_boxstats_f64 as it is: -> (sorted: the doubles group by group, ascending inside a group; boxes: a BOX record per group that
    occurs, ascending in group)"""
    k, v = np.ascontiguousarray(key, dtype=np.uint32), np.ascontiguousarray(x, dtype=np.float64)
    if k.shape != v.shape or k.ndim != 1:
        raise ValueError("one value per key")
    lib, n = _lib(lib), k.size
    out, cap = np.empty(n, dtype=np.float64), min(n, BOX_CAP_FIRST)
    while True:
        boxes, nb, err = np.zeros(cap, dtype=BOX), C.c_uint32(0), C.create_string_buffer(512)
        rc = lib.lqfig_boxstats_f64(device, _ptr(k), _ptr(v), n, float(interval), float(whis), _ptr(out), _ptr(boxes), cap, C.byref(nb), err, 512)
        if rc == -1 and nb.value > cap:                             # (LQCOV_E_ARG with the number of groups: once more with room for them)
            cap = nb.value
            continue
        if rc != 0:
            raise api.LqcovError(rc, err.value.decode())
        return out, boxes[:nb.value]


def box_stats_f64(key, x, interval: float = 0.0, whis: float = 1.5, device: int = 0, lib=None) -> dict:
    """matplotlib.cbook.boxplot_stats(x, whis) of every group of doubles, on the device (kernels_boxstats_f64.hpp); the group of element i
    is key[i], or with an interval np.floor(key[i] / interval).  -> a dict of arrays with one entry per group that occurs, ascending in
    group: group, n, q1, med, q3, whislo, whishi, median, and fliers, a list of arrays (below whislo, then above whishi, ascending)"""
    return _box_dict(*box_stats_f64_raw(key, x, interval, whis, device, lib))


# ---- the host's small parts -----------------------------------------------------------------------------------------------------------
def parse_sts_xml(filepath, ns=STS_NS):
    """[P0, P1, P2] of an RS-II *.sts.xml: BinCount and BinLabel are direct children of ProdDist and are paired by position; a label that
    contains Empty, else Productive, else Other gives P0, P1, P2 (0 for one that does not occur; of two bins with one label the later)"""
    root = et.parse(filepath).getroot()
    bc = root.findall("./{%s}ProdDist/{%s}BinCount" % (ns, ns))
    bl = root.findall("./{%s}ProdDist/{%s}BinLabel" % (ns, ns))
    p = [0, 0, 0]
    for i, label in enumerate(bl):
        which = next((k for k, word in enumerate(("Empty", "Productive", "Other")) if word in label.text), None)
        if which is not None:
            p[which] = int(bc[i].text)
    return p


def _first_with_suffix(d, suffix):
    if not os.path.isdir(d):
        return None
    for name in os.listdir(d):
        if name.endswith(suffix):
            return os.path.join(d, name)
    return None


def get_sts_xml_path(d):
    """the first name os.listdir gives that ends in .sts.xml, or None (lq_rs.get_sts_xml_path)"""
    return _first_with_suffix(d, ".sts.xml")


def get_sts_csv_path(d):
    """the first name os.listdir gives that ends in .sts.csv, or None (lq_rs.get_sts_csv_path)"""
    return _first_with_suffix(d, ".sts.csv")


# ---- the device part ------------------------------------------------------------------------------------------------------------------
class StsTable:
    """A comma-separated table on the device.  source: a path, the file's bytes, or a list of its bytes in parts; columns: (name, INT64 | DOUBLE) pairs, the header
    columns to read.  Afterwards n_rows, stats (a dict of STATS), column(name) -> the int64 or float64 array as pd.read_table gives it
    for a column of that type, and the RS-II statistics: lengths(), hist(), log_sums(), get_lengths(), box_stats().  piece_bytes: the size
    of an upload piece (tests: pieces shorter than a row)."""

    def __init__(self, source, columns=COLUMNS, device: int = 0, piece_bytes=None, lib=None):
        self.h = None                                               # (close() may run before the handle exists)
        self.lib = _lib(lib)
        self.device = device
        self.columns = [(str(n), int(k)) for n, k in columns]
        self.h = self.lib.lqcsv_create(device)
        if not self.h:
            raise api.LqcovError(-3, self.lib.lqcsv_last_error(None).decode())
        try:
            for name, kind in self.columns:
                self._check(self.lib.lqcsv_want(self.h, name.encode(), kind))
            if piece_bytes is not None:
                self._check(self.lib.lqcsv_set_piece_bytes(self.h, int(piece_bytes)))
            if isinstance(source, (bytes, bytearray, memoryview)):
                source = [bytes(source)]
            if isinstance(source, (list, tuple)):                   # the file's bytes as they arrive: what a call leaves goes in front of the next
                left, r = b"", C.c_uint64(0)
                for k, part in enumerate(source):
                    buf = np.frombuffer(left + bytes(part), dtype=np.uint8)
                    self._check(self.lib.lqcsv_add_bytes(self.h, _ptr(buf), buf.size, int(k + 1 == len(source)), C.byref(r)))
                    left = buf[r.value:].tobytes()
            else:
                self._check(self.lib.lqcsv_add_file(self.h, os.fsencode(source)))
            n = C.c_uint64(0)
            self._check(self.lib.lqcsv_finish(self.h, C.byref(n)))
        except BaseException:
            self.close()
            raise
        self.n_rows = int(n.value)
        st = (C.c_uint64 * len(STATS))()
        self._check(self.lib.lqcsv_stats(self.h, st))
        self.stats = dict(zip(STATS, (int(x) for x in st)))
        self.length_stats = None

    def close(self):
        if self.h:
            self.lib.lqcsv_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise api.LqcovError(rc, self.lib.lqcsv_last_error(self.h).decode())

    def _col(self, name):
        for i, (n, _) in enumerate(self.columns):
            if n == name:
                return i
        raise KeyError(name)

    def column(self, name):
        i = self._col(name)
        out = np.zeros(self.n_rows, dtype=np.int64 if self.columns[i][1] == INT64 else np.float64)
        self._check(self.lib.lqcsv_get(self.h, i, _ptr(out)))
        return out

    def lengths(self, score="ReadScore", threshold=0.1, start="HQRegionStart", end="HQRegionEnd", bases="NumBases"):
        """end - start of every row, and under the mask score > threshold the lengths and the bases compacted, their sums, minima and
        maxima, N50 and N90: -> a dict of LENGTHS.  LqcovError where a length lies below 0 or above 2^32-1"""
        w = (C.c_uint64 * len(LENGTHS))()
        self._check(self.lib.lqcsv_lengths(self.h, self._col(score), float(threshold), self._col(start), self._col(end), self._col(bases), w))
        self.length_stats = dict(zip(LENGTHS[:-1], (int(x) for x in w)))
        return self.length_stats

    def get_lengths(self, which):
        """the resident uint32 array: HQ or BASES (the masked rows), LEN_ALL (every row)"""
        out = np.zeros(self.n_rows if which == LEN_ALL else (self.length_stats or {"n": 0})["n"], dtype=np.uint32)
        self._check(self.lib.lqcsv_get_lengths(self.h, which, _ptr(out)))
        return out

    def hist(self, which, edges):
        """np.histogram(the resident array, bins=edges)[0]"""
        e = np.ascontiguousarray(edges, dtype=np.float64)
        counts = np.zeros(max(e.size - 1, 0), dtype=np.uint64)
        self._check(self.lib.lqcsv_hist(self.h, which, _ptr(e), e.size, _ptr(counts)))
        return counts.astype(np.int64)

    def log_sums(self):
        """(sum, sum of log over the non-zero values, number of zeros) of the masked lengths, on the device"""
        s, z, sl = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        self._check(self.lib.lqcsv_logsum(self.h, C.byref(s), C.byref(sl), C.byref(z)))
        return int(s.value), float(sl.value), int(z.value)

    def box_stats(self, value="ReadScore", interval=1000.0, whis=1.5):
        """df.boxplot(column=value, by=np.floor(length / interval)) over every row: box_stats_f64's dict, from the resident columns"""
        n, i = self.n_rows, self._col(value)
        out, cap = np.empty(n, dtype=np.float64), min(n, BOX_CAP_FIRST)
        while True:
            boxes, nb = np.zeros(cap, dtype=BOX), C.c_uint32(0)
            rc = self.lib.lqcsv_boxstats(self.h, i, float(interval), float(whis), _ptr(out), _ptr(boxes), cap, C.byref(nb))
            if rc == -1 and nb.value > cap:
                cap = nb.value
                continue
            self._check(rc)
            return _box_dict(out, boxes[:nb.value])


def run_platformqc(data_path, output_path=None, suffix=None, b_width=1000, device: int = 0, lib=None):
    """lq_rs.run_platformqc -> (the JSON block as a dict, what the two figures plot).  With output_path, QC_vals_rs<_suffix>.json is
    written there as the reference writes it.  A missing sts.xml gives Productivity of three None.  A missing sts.csv raises
    FileNotFoundError (the reference crashes there, on `logger.ERROR`, which is no method of a logger); no row with ReadScore > 0.1 raises
    ValueError as the reference's max() of an empty array does; a negative HQRegionEnd - HQRegionStart raises LqcovError"""
    suffix = "_" + suffix if suffix else ""
    xml_file = get_sts_xml_path(data_path)
    productivity = parse_sts_xml(xml_file) if xml_file else [None] * 3
    csv_path = get_sts_csv_path(data_path)
    if not csv_path:
        raise FileNotFoundError("Platform QC failed due to missing csv files: no *.sts.csv in %s" % data_path)
    with StsTable(csv_path, device=device, lib=lib) as t:
        st = t.lengths()
        n = st["n"]
        if not n:
            raise ValueError("no row has a ReadScore above 0.1: max() of an empty array")
        s, sum_log, zeros = t.log_sums()
        if zeros:
            raise ValueError("%d HQ regions have a length of 0: gamma.fit(floc=0) needs positive data" % zeros)
        a, b = figdata.gamma_fit(n, s, sum_log)
        hq, bases = t.get_lengths(HQ), t.get_lengths(BASES)
        with np.errstate(divide="ignore", invalid="ignore"):
            fracs = hq / bases                                      # (on the host, as sequel.py takes its fractions)
        js = {
            "Productivity": {"P0": productivity[0], "P1": productivity[1], "P2": productivity[2]},
            "Throughput": int(st["sum_hq"]),
            "Longest_read": int(st["max_hq"]),
            "Num_of_reads": int(n),
            "polread_gamma_params": [float(a), float(b)],
            "Mean_polread_length": float(st["sum_hq"] / n),
            "N50_polread_length": float(st["n50"]),
            "Mean_HQ_fraction": float(np.mean(fracs)),
        }
        fig = {}
        for key, which, lo, hi in (("hq", HQ, st["min_hq"], st["max_hq"]), ("bases", BASES, st["min_bases"], st["max_bases"])):
            edges, counts, density = figdata.density_hist(None, lo, hi + b_width, b_width, hist_fn=lambda e, w=which: t.hist(w, e))
            fig[key + "_edges"], fig[key + "_counts"], fig[key + "_density"] = edges, counts, density
        fig.update(gamma_a=float(a), gamma_b=float(b), mean=float(st["sum_hq"] / n), n50=float(st["n50"]), n90=float(st["n90"]))
        fig["box"] = t.box_stats("ReadScore", b_width)
        fig.update(hq_lengths=hq, num_bases=bases, stats=dict(t.stats), lengths=dict(st))
    if output_path is not None:
        os.makedirs(output_path, exist_ok=True)
        with open(os.path.join(output_path, "QC_vals_rs" + suffix + ".json"), "w") as f:
            json.dump(js, f, indent=4)
    return js, fig

"""LongQC's `runqc -p sequel` on the device: what lq_sequel.run_platformqc (lq_sequel.py:207-379) computes from the *.scraps.bam and
*.subreads.bam of a Sequel run -- the polymerase read of every ZMW (construct_polread), their length and adapter statistics, the gamma
fit, N50 / N90 and the two length histograms -- without pysam, scipy or matplotlib.  The records are found, read, ordered and walked on
the device (kernels_polread.hpp behind lqpol_* of include/lqcov.h); the host reads the BAM headers' text, the sts.xml and a few numbers.
Nothing is drawn: figure_data() returns what the two figures plot.  No CPU fallback: without liblqcov.so or a HIP device the calls raise.

    js, fig = run_platformqc(run_dir, out_dir)        # out_dir/QC_vals_sequel.json is written; js is its content

A caller with another source of items uses polymerase_reads(items) or PolymeraseReads.add_items."""
import ctypes as C
import json
import os
import xml.etree.ElementTree as et

import numpy as np

from . import api, chunkpass, figdata

STATS = ("sum_hq", "max_hq", "min_tot", "max_tot", "n50", "n90", "n_tot_zero", "min_ad", "max_ad", "n_long_zmw",
         "records_device", "records_flagged", "records_host", "bytes_inflated", "bytes_to_host", "pieces", "n_out_of_range")
INFLATE_MODES = {"host": 0, "device": 1}
HQ, TOT, AD = 0, 1, 2                                              # LQPOL_HQ / LQPOL_TOT / LQPOL_AD
STS_NS = "http://pacificbiosciences.com/PacBioPipelineStats.xsd"
STS_BASE_NS = "http://pacificbiosciences.com/PacBioBaseDataModel.xsd"


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqpol_bound", False):
        H, v, u64, tail = C.c_void_p, C.c_void_p, C.c_uint64, [C.c_char_p, C.c_size_t]
        lib.lqpol_create.restype, lib.lqpol_create.argtypes = H, [C.c_int]
        lib.lqpol_destroy.restype, lib.lqpol_destroy.argtypes = None, [H]
        lib.lqpol_last_error.restype, lib.lqpol_last_error.argtypes = C.c_char_p, [H]
        for name, args in (("lqpol_add_bytes", [H, C.c_int, v, u64, u64, v]), ("lqpol_add_file", [H, C.c_int, C.c_char_p, C.c_int, C.c_int]),
                           ("lqpol_header_text", [H, C.c_int, v, u64, v]), ("lqpol_file_header", [C.c_char_p, v, u64, v] + tail), ("lqpol_add_items", [H, v, v, v, v, u64]),
                           ("lqpol_finish", [H, v, v, v]), ("lqpol_get", [H, v, v, v, v, v]), ("lqpol_stats", [H, v]),
                           ("lqpol_hist", [H, C.c_int, v, C.c_uint32, v]), ("lqpol_logsum", [H, v, v, v]),
                           ("lqpol_fields", [C.c_int, C.c_int, v, u64, u64, v, v, u64, v, v, v, v] + tail),
                           ("lqpol_twin", [C.c_int, v, u64, u64, v, v, v] + tail)):
            f = getattr(lib, name)
            f.restype, f.argtypes = C.c_int, args
        lib._lqpol_bound = True
    return lib


def inflate_mode(inflate):
    """"host" | "device" | None (the environment variable LQREADER_INFLATE, "host" without it) -> the mode's name"""
    mode = os.environ.get("LQREADER_INFLATE", "host") if inflate is None else inflate
    if mode not in INFLATE_MODES:
        raise ValueError("inflate must be 'host' or 'device', not %r" % (mode,))
    return mode


# ---- the host's small parts ---------------------------------------------------------------------------------------------------------
def _rg_descriptions(header_text):
    """the DS field of every @RG line of a BAM header's text, in file order"""
    if isinstance(header_text, bytes):
        header_text = header_text.decode("ascii", "replace")
    for line in header_text.splitlines():
        tag, *fields = line.split("\t")
        if tag == "@RG":
            ds = [f[3:] for f in fields if f.startswith("DS:")]
            if ds:
                yield ds[-1]                                        # (a dict of the line's fields keeps the last of a repeated key)


def get_readtype(header_text):
    """The READTYPE a PacBio BAM declares: the value of the first `READTYPE=...` entry among the `;`-separated entries of the first
    @RG description that mentions READTYPE at all; None if no read group does.  header_text: the header's text, str or bytes"""
    for ds in _rg_descriptions(header_text):
        if "READTYPE" not in ds:
            continue
        for entry in ds.split(";"):
            key, eq, rest = entry.partition("=")
            if key == "READTYPE" and eq:
                return rest.split("=")[0]
    return None


PRODUCTIVITY_LABELS = ("Empty", "Productive", "Other")            # P0, P1, P2: a bin belongs to the first of these its label contains


def parse_sts_xml(filepath, ns=STS_BASE_NS):
    """[P0, P1, P2] of a *.sts.xml: the ProdDist bin counts whose labels read Empty, Productive and Other (0 for a label that does not
    occur; of two bins with one label the later counts).  Labels and counts are paired by their position under BinLabels / BinCounts"""
    dist = et.parse(filepath).getroot().find("./{%s}ProdDist" % STS_NS)
    labels, counts = (dist.find("{%s}%s" % (ns, name)) for name in ("BinLabels", "BinCounts"))
    productivity = dict.fromkeys(PRODUCTIVITY_LABELS, 0)
    for label, count in zip(labels, counts):
        if "BinLabel" not in label.tag:
            continue
        which = next((k for k in PRODUCTIVITY_LABELS if k in label.text), None)
        if which is not None:
            productivity[which] = int(count.text)
    return [productivity[k] for k in PRODUCTIVITY_LABELS]


def _last_with_suffix(d, suffix):
    found = None
    for name in os.listdir(d):
        p = os.path.join(d, name)
        if not os.path.isdir(p) and p.endswith(suffix):
            found = p
    return found


def get_sts_xml_path(d):
    """the directory's *.sts.xml, or None (lq_sequel.get_sts_xml_path returns the first that os.listdir names)"""
    if not os.path.isdir(d):
        return None
    for name in os.listdir(d):
        if name.endswith(".sts.xml"):
            return os.path.join(d, name)
    return None


def get_bam_path(d):
    """[subreads path, scraps path] of a run directory (lq_sequel.get_bam_path); FileNotFoundError where the reference gives up: d is no
    directory, or one of the two files is missing"""
    if not os.path.isdir(d):
        raise FileNotFoundError("%s is not a dir" % d)
    subreads, scraps = _last_with_suffix(d, ".subreads.bam"), _last_with_suffix(d, ".scraps.bam")
    if not subreads or not scraps:
        raise FileNotFoundError("bam files are missing in %s: %s" % (d, " and ".join(n for n, p in (("*.subreads.bam", subreads), ("*.scraps.bam", scraps)) if not p)))
    return [subreads, scraps]


def file_header(path, lib=None):
    """the header text (bytes) of a BAM file, inflated from its first blocks on the host; nothing else of the file is read"""
    lib = _lib(lib)
    n, err = C.c_uint64(0), C.create_string_buffer(768)
    for _ in range(2):                                              # the length, then the text
        buf = C.create_string_buffer(n.value + 1)
        rc = lib.lqpol_file_header(os.fsencode(path), buf, n.value, C.byref(n), err, 768)
        if rc != 0:
            raise api.LqcovError(rc, err.value.decode())
    return buf.raw[:n.value]


# ---- the device part ----------------------------------------------------------------------------------------------------------------
class PolymeraseReads:
    """The polymerase reads of one run.  add_scraps(path), add_subreads(path) -- in that order, as the reference loads them -- or
    add_items(...); then finish().  Afterwards, over the ZMWs that hold a subread (is_pol), in ascending ZMW order: zmw, hr_lengths (hq),
    tot_lengths, hr_fraction, ad_num, ad_num_stat {ad_num: count}; control_throughput; all_zmw / all_hq / all_tot / all_ad_num / is_pol over
    every ZMW; stats, a dict of STATS.  inflate: "host" | "device" | None (LQREADER_INFLATE); host_copy: "all" | "needed" | None
    (LQREADER_HOSTCOPY): with device inflate and "needed" the inflated bytes never leave the device."""

    def __init__(self, device: int = 0, inflate=None, host_copy=None, lib=None):
        self.h = None                                               # (close() may run before the handle exists)
        self.lib = _lib(lib)
        self.device = device
        self.inflate, self.host_copy = inflate_mode(inflate), chunkpass.host_copy_mode(host_copy)
        self.h = self.lib.lqpol_create(device)
        if not self.h:
            raise api.LqcovError(-3, self.lib.lqpol_last_error(None).decode())
        self.finished = False
        self.headers = {}

    def close(self):
        if self.h:
            self.lib.lqpol_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise api.LqcovError(rc, self.lib.lqpol_last_error(self.h).decode())

    def _add_file(self, kind, path, want):
        got = get_readtype(file_header(path, self.lib))             # from the file's first blocks: before anything is read or added
        if got != want:
            raise ValueError("%s: the header's READTYPE is %r, not %r" % (path, got, want))
        self._check(self.lib.lqpol_add_file(self.h, kind, os.fsencode(path), INFLATE_MODES[self.inflate], chunkpass.HOSTCOPY_MODES[self.host_copy]))
        n = C.c_uint64(0)
        self.lib.lqpol_header_text(self.h, kind, None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value + 1)
        self.lib.lqpol_header_text(self.h, kind, buf, n.value, C.byref(n))
        self.headers[kind] = buf.raw[:n.value]

    def add_scraps(self, path):
        self._add_file(0, path, "SCRAP")

    def add_subreads(self, path):
        self._add_file(1, path, "SUBREAD")

    def add_bytes(self, kind, data, start_pos=0):
        """inflated BAM bytes, a parser at start_pos behind the header -> the position of the first record that is not whole"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        r = C.c_uint64(0)
        self._check(self.lib.lqpol_add_bytes(self.h, kind, buf.ctypes.data if buf.size else None, buf.size, int(start_pos), C.byref(r)))
        return r.value

    def add_items(self, zmw, start, end, cls):
        """items given directly; cls: class letters as bytes / str of length n, or an array of their codes"""
        z, s, e = (np.ascontiguousarray(a, dtype=np.uint32) for a in (zmw, start, end))
        c = np.frombuffer(cls.encode() if isinstance(cls, str) else bytes(cls), dtype=np.uint8) if isinstance(cls, (str, bytes, bytearray)) else np.ascontiguousarray(cls, dtype=np.uint8)
        if not (z.shape == s.shape == e.shape == c.shape) or z.ndim != 1:
            raise ValueError("one zmw, start, end and class per item")
        self._check(self.lib.lqpol_add_items(self.h, z.ctypes.data, s.ctypes.data, e.ctypes.data, c.ctypes.data, z.size))

    def finish(self):
        n_zmw, n_pol, control = C.c_uint64(0), C.c_uint64(0), C.c_int64(0)
        self._check(self.lib.lqpol_finish(self.h, C.byref(n_zmw), C.byref(n_pol), C.byref(control)))
        n = n_zmw.value
        self.all_zmw, self.all_hq, self.all_tot = np.zeros(n, np.uint32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.all_ad_num, pol = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._check(self.lib.lqpol_get(self.h, self.all_zmw.ctypes.data, self.all_hq.ctypes.data, self.all_tot.ctypes.data, self.all_ad_num.ctypes.data, pol.ctypes.data))
        st = (C.c_uint64 * len(STATS))()
        self._check(self.lib.lqpol_stats(self.h, st))
        self.stats = dict(zip(STATS, (int(x) for x in st)))
        self.is_pol = pol.astype(bool)
        self.control_throughput = int(control.value)
        self.n_pol = int(n_pol.value)
        self.zmw, self.hr_lengths, self.tot_lengths = self.all_zmw[self.is_pol], self.all_hq[self.is_pol], self.all_tot[self.is_pol]
        self.ad_num = self.all_ad_num[self.is_pol]
        self.hr_fraction, self.ad_num_stat = None, {}
        self.finished = True
        if self.stats["n_tot_zero"]:                                # (the per-ZMW integers stand; _need_reads refuses the rest)
            raise ZeroDivisionError("%d polymerase reads have a total length of 0: the reference divides by it" % self.stats["n_tot_zero"])
        self.hr_fraction = self.hr_lengths / self.tot_lengths
        if self.n_pol and not self.stats["n_out_of_range"]:
            lo, hi = self.stats["min_ad"], self.stats["max_ad"]
            counts = self.hist(AD, np.arange(lo, hi + 2, dtype=np.float64))
            self.ad_num_stat = {lo + k: int(c) for k, c in enumerate(counts) if c}
        return self

    def hist(self, which, edges):
        """np.histogram(the resident array, bins=edges)[0]: which = HQ, TOT or AD"""
        e = np.ascontiguousarray(edges, dtype=np.float64)
        counts = np.zeros(max(e.size - 1, 0), dtype=np.uint64)
        self._check(self.lib.lqpol_hist(self.h, which, e.ctypes.data if e.size else None, e.size, counts.ctypes.data if counts.size else None))
        return counts.astype(np.int64)

    def log_sums(self):
        """(sum, sum of log over the non-zero values, number of zeros) of hr_lengths, on the device"""
        s, z, sl = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        self._check(self.lib.lqpol_logsum(self.h, C.byref(s), C.byref(sl), C.byref(z)))
        return int(s.value), float(sl.value), int(z.value)

    def gamma_params(self):
        """gamma.fit(hr_lengths, floc=0) -> (a, scale).  ValueError where scipy raises: no reads, a read of length 0 (scipy: "The data
        contains non-positive values"), lengths without spread"""
        if not self.n_pol:
            raise ValueError("no polymerase reads to fit")
        s, sl, zeros = self.log_sums()
        if zeros:
            raise ValueError("%d polymerase reads have an HQ length of 0: gamma.fit(floc=0) needs positive data" % zeros)
        return figdata.gamma_fit(self.n_pol, s, sl)

    def _need_reads(self):
        if not self.finished:
            raise RuntimeError("finish() has not been called")
        if not self.n_pol:
            raise ValueError("no ZMW holds a subread: max() arg is an empty sequence")
        if self.stats["n_tot_zero"]:
            raise ZeroDivisionError("%d polymerase reads have a total length of 0: the reference divides by it" % self.stats["n_tot_zero"])
        if self.stats["n_out_of_range"]:
            raise api.LqcovError(-5, "%d polymerase reads with a length below 0 or above 2^32-1" % self.stats["n_out_of_range"])

    def json_block(self, productivity=None):
        """the dict run_platformqc dumps (lq_sequel.py:327-336), with its keys and Python types"""
        self._need_reads()
        st = self.stats
        a, b = self.gamma_params()
        p = [None] * 3 if productivity is None else list(productivity)
        return {
            "Productivity": {"P0": p[0], "P1": p[1], "P2": p[2]},
            "Throughput": int(st["sum_hq"]),
            "Throughput(Control)": int(self.control_throughput),
            "Longest_read": int(st["max_hq"]),
            "Num_of_reads": int(self.n_pol),
            "polread_gamma_params": [float(a), float(b)],
            "Mean_polread_length": float(st["sum_hq"] / self.n_pol),
            "N50_polread_length": float(st["n50"]),
            "Mean_HQ_fraction": float(np.mean(self.hr_fraction)),
            "Adapter_observation": dict(self.ad_num_stat),
        }

    def figure_data(self, b_width=1000):
        """what the two figures plot: the adapter bars (left, height over min .. max of ad_num), np.histogram(..., density=True) of
        hr_lengths and of tot_lengths over np.arange(min, max + b_width, b_width), the gamma curve's parameters, mean, N50 and N90"""
        self._need_reads()
        st = self.stats
        lo, hi = st["min_ad"], st["max_ad"]
        out = {"adapter_left": list(range(lo, hi + 1)), "adapter_height": [self.ad_num_stat.get(i, 0) for i in range(lo, hi + 1)]}
        hq_min = int(self.hr_lengths.min())
        for key, which, start, stop in (("hr", HQ, hq_min, st["max_hq"] + b_width), ("tot", TOT, st["min_tot"], st["max_tot"] + b_width)):
            edges, counts, density = figdata.density_hist(None, start, stop, b_width, hist_fn=lambda e, w=which: self.hist(w, e))
            out[key + "_edges"], out[key + "_counts"], out[key + "_density"] = edges, counts, density
        a, b = self.gamma_params()
        out.update(gamma_a=float(a), gamma_b=float(b), mean=float(st["sum_hq"] / self.n_pol), n50=float(st["n50"]), n90=float(st["n90"]))
        out.update(hr_lengths=self.hr_lengths, tot_lengths=self.tot_lengths, stats=dict(st))      # (the arrays behind the histograms; how the run went)
        return out


def polymerase_reads(items, device: int = 0, lib=None):
    """construct_polread over items given directly: items = {zmw: [(start, end, class letter), ...]} or a list of (zmw, start, end, class)
    in arrival order -> {zmw: (hq, tot, is_pol, ad_num)} for every ZMW"""
    if isinstance(items, dict):
        items = [(z, s, e, c) for z, l in items.items() for s, e, c in l]
    with PolymeraseReads(device, lib=lib) as p:
        if items:
            z, s, e, c = zip(*items)
            p.add_items(np.array(z, np.int64), np.array(s, np.int64), np.array(e, np.int64), "".join(c))
        _finish_lenient(p)
        return {int(z): (int(h), int(t), bool(i), int(a)) for z, h, t, i, a in zip(p.all_zmw, p.all_hq, p.all_tot, p.is_pol, p.all_ad_num)}


def _finish_lenient(p):
    try:
        p.finish()
    except ZeroDivisionError:
        pass                                                       # (the per-ZMW integers are there; only hq / tot is not)


def run_platformqc(data_path, output_path=None, suffix=None, b_width=1000, device: int = 0, inflate=None, host_copy=None, lib=None):
    """lq_sequel.run_platformqc -> (the JSON block as a dict, figure_data()).  With output_path, QC_vals_sequel<_suffix>.json is written
    there as the reference writes it.  A missing sts.xml gives Productivity of three None; a missing BAM raises FileNotFoundError, a file
    whose header names another READTYPE raises ValueError"""
    suffix = "_" + suffix if suffix else ""
    xml_file = get_sts_xml_path(data_path)
    productivity = parse_sts_xml(xml_file) if xml_file else [None] * 3
    subreads, scraps = get_bam_path(data_path)
    with PolymeraseReads(device, inflate, host_copy, lib) as p:
        p.add_scraps(scraps)
        p.add_subreads(subreads)
        p.finish()
        js, fig = p.json_block(productivity), p.figure_data(b_width)
    if output_path is not None:
        os.makedirs(output_path, exist_ok=True)
        with open(os.path.join(output_path, "QC_vals_sequel" + suffix + ".json"), "w") as f:
            json.dump(js, f, indent=4)
    return js, fig

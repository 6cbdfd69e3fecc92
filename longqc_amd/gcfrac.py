"""The GC fraction step of LongQC's sampleqc (lq_gcfrac.py:15-48 `LqGC.calc_read_and_chunk_gc_frac`, driven by
longQC.py:284,328,449,504-506) over the C ABI of include/lqcov.h (lqgc_reads): the G/C counts of the reads and of the sampled
`chunk_size`-base windows are made on the device (kernels_gc.hpp) and come back as integers; the divisions, the float32
roundings of `array('f')` and the totals are made here with the reference's operations.  No CPU fallback: without
liblqcov.so or a HIP device the calls raise.

The sampled positions (`np.random.choice(l, k, replace=False)` in the reference, never seeded there) come from one of two
draws: draw="numpy" calls np.random.choice per read on the host, in read order, as the reference does -- after
np.random.seed(x) the object equals the reference's after the same seed; draw="device" evaluates a bijection of [0, l) keyed by
(seed, the read's ordinal in the whole input) on the device: fast, reproducible, and independent of how the
input was cut into chunks.  plot_unmasked_gc_frac's figure is not drawn; figure_data() returns the numbers behind it -- the two
histograms and the two KDE curves, made on the device over every read and window (longqc_amd/figdata.py) -- for the caller to plot."""
import array
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import api


def _lib(lib=None):
    lib = lib or api.load_library()
    if not getattr(lib, "_lqgc_bound", False):
        lib.lqgc_reads.restype = C.c_int
        lib.lqgc_reads.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib._lqgc_bound = True
    return lib


def draws_per_read(lens: np.ndarray, chunk_size: int, samp_rate: float) -> np.ndarray:
    """int(float(1/chunk_size) * l * samp_rate) of lq_gcfrac.py:38 per read, as int64: the same two float64 products in the same
    order, truncated"""
    x = np.float64(1 / chunk_size) * np.asarray(lens).astype(np.float64) * np.float64(samp_rate)
    return np.trunc(x).astype(np.int64)


def _flatten(seqs: Sequence) -> Tuple[bytes, np.ndarray]:
    n = len(seqs)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.uint64, count=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = "".join(seqs).encode("latin-1") if n and isinstance(seqs[0], str) else b"".join(bytes(s) for s in seqs)
    if len(flat) != int(off[n]):
        raise ValueError("reads must be all str or all bytes")
    return flat, off


def _call(lib, device, flat, off, chunk_size, k, pos_in, seed, first_read, chunk=None):
    """lqgc_reads on flat buffers -- or lqchunk_gc on a chunkpass.ReadChunk, flat and off then unused -- -> (gc, pos, win_gc, kept);
    pos / win_gc / kept are None when k is None"""
    n = chunk.n if chunk is not None else int(off.shape[0] - 1)
    gc = np.zeros(max(n, 1), dtype=np.uint32)
    doff = pos = win = kept = None
    if k is not None:
        k = np.ascontiguousarray(k, dtype=np.uint32)
        doff = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(k, out=doff[1:], dtype=np.uint64)
        nd = int(doff[n])
        if pos_in is not None:
            pos_in = np.ascontiguousarray(pos_in, dtype=np.uint32)
            if pos_in.shape != (nd,):
                raise ValueError("pos_in must hold sum(k) positions")
        pos = np.zeros(max(nd, 1), dtype=np.uint32)
        win = np.zeros(max(nd, 1), dtype=np.uint16)
        kept = np.zeros(max(n, 1), dtype=np.uint32)
    tail = (k.ctypes.data if k is not None else None, doff.ctypes.data if k is not None else None,
            pos_in.ctypes.data if pos_in is not None else None, seed, first_read, gc.ctypes.data,
            pos.ctypes.data if k is not None else None, win.ctypes.data if k is not None else None,
            kept.ctypes.data if k is not None else None)
    if chunk is not None:
        chunk.gc(chunk_size, *tail)
    else:
        err = C.create_string_buffer(512)
        rc = _lib(lib).lqgc_reads(device, n, flat if len(flat) else None, off.ctypes.data, chunk_size, *tail, err, 512)
        if rc != 0:
            raise api.LqcovError(rc, err.value.decode())
    if k is None:
        return gc[:n], None, None, None
    return gc[:n], pos[:nd], win[:nd], kept[:n]


def gc_counts(seqs: Sequence, chunk_size: int = 150, k=None, pos_in=None, seed: int = 0, first_read: int = 0, device: int = 0, lib=None):
    """The array-level call.  seqs: the reads, all str or all bytes.  -> (gc, pos, win_gc, kept): gc[i] the 'G' + 'C' bytes of
    read i; with k (draws per read): pos the positions used, read after read in draw order (pos_in's, or the device draw of
    (seed, first_read + i)), kept[i] the index of the first position p of read i with p + chunk_size - 1 > len (or k[i]),
    win_gc[d] the G/C bytes of seq[p : p + chunk_size] for the draws before kept[i], 0 for the others.  Without k the last three
    are None."""
    flat, off = _flatten(seqs)
    return _call(lib, device, flat, off, chunk_size, k, pos_in, seed, first_read)


class LqGCMI355X:
    """LqGC of lq_gcfrac.py:15-48: the same attributes, calc_read_and_chunk_gc_frac called once per chunk and accumulating.
    gc_stats() is what plot_unmasked_gc_frac returns, json_block() the `GC_stats` entry of longQC.py:504-506."""

    def __init__(self, chunk_size=150, draw="device", seed=0, device=0, lib=None):
        if draw not in ("device", "numpy"):
            raise ValueError("draw must be 'device' or 'numpy'")
        self.chunk_size = chunk_size
        self.r_frac = array.array('f')
        self.c_frac = array.array('f')
        self.r_tot = 0
        self.c_tot = 0
        self.r_gc_tot = 0
        self.c_gc_tot = 0
        self.draw, self.seed, self.device, self.lib = draw, seed, device, lib
        self.n_reads = 0                                           # reads seen so far: the ordinal of the next chunk's first read
        self.last_pos = None                                       # the last call's positions, read after read in draw order

    def calc_read_and_chunk_gc_frac(self, reads, samp_rate=0.2, chunk=None):
        """reads: LongQC's [name, seq, ...] records (seq str or bytes, upper case as the reference expects).  A read without
        bases raises ZeroDivisionError and one with more draws than bases ValueError, where the reference does, with the reads
        before it (and, for ValueError, its own read-level numbers) accumulated as the reference leaves them.
        chunk: the chunkpass.ReadChunk made of `reads`: the counts come from its device copy, nothing is gathered or uploaded."""
        cs = self.chunk_size
        if chunk is not None:
            return self._calc_on_chunk(chunk, samp_rate)
        seqs = [r[1] for r in reads]
        n = len(seqs)
        lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=n)
        k = draws_per_read(lens, cs, samp_rate)
        bad = np.flatnonzero((lens == 0) | (k > lens) | (k < 0))
        stop = int(bad[0]) if bad.size else n                      # the reference's loop ends inside read `stop`
        n_read_level = stop + 1 if stop < n and lens[stop] > 0 else stop      # ValueError comes after the read-level updates
        seqs, lens, k = seqs[:n_read_level], lens[:n_read_level], k[:n_read_level].copy()
        k[stop:] = 0
        flat, off = _flatten(seqs)
        pos_in = None
        if self.draw == "numpy":                                   # the reference's stream: one call per read, k == 0 included
            drawn = [np.random.choice(int(lens[i]), int(k[i]), replace=False) for i in range(stop)]
            pos_in = np.concatenate(drawn).astype(np.uint32) if drawn else np.zeros(0, dtype=np.uint32)
        gc, self.last_pos, win, kept = _call(self.lib, self.device, flat, off, cs, k.astype(np.uint32), pos_in, self.seed, self.n_reads)
        self._accumulate(n, stop, n_read_level, lens, k, gc, win, kept, samp_rate)

    def _calc_on_chunk(self, chunk, samp_rate):
        """the same on a resident chunk: every read of the chunk is counted, the reads behind the one the reference's loop ends in
        draw nothing and are left out of the sums"""
        cs, n, lens = self.chunk_size, chunk.n, chunk.lens
        k = draws_per_read(lens, cs, samp_rate)
        bad = np.flatnonzero((lens == 0) | (k > lens) | (k < 0))
        stop = int(bad[0]) if bad.size else n
        n_read_level = stop + 1 if stop < n and lens[stop] > 0 else stop
        k = k.copy()
        k[stop:] = 0
        pos_in = None
        if self.draw == "numpy":
            drawn = [np.random.choice(int(lens[i]), int(k[i]), replace=False) for i in range(stop)]
            pos_in = np.concatenate(drawn).astype(np.uint32) if drawn else np.zeros(0, dtype=np.uint32)
        gc, self.last_pos, win, kept = _call(self.lib, self.device, None, None, cs, k.astype(np.uint32), pos_in, self.seed, self.n_reads, chunk=chunk)
        self._accumulate(n, stop, n_read_level, lens[:n_read_level], k[:n_read_level], gc[:n_read_level], win, kept[:n_read_level], samp_rate)

    def _accumulate(self, n, stop, n_read_level, lens, k, gc, win, kept, samp_rate):
        cs = self.chunk_size
        self.n_reads += stop
        # gc_n / l: the correctly rounded float64 quotient of two integers, rounded once more by array('f')
        self.r_frac.frombytes((gc.astype(np.float64) / lens.astype(np.float64)).astype(np.float32).tobytes())
        self.r_tot += int(lens.sum())
        self.r_gc_tot += int(gc.sum(dtype=np.int64))
        j = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(np.cumsum(k) - k, k)       # a draw's index within its read
        taken = win[j < np.repeat(kept.astype(np.int64), k)]
        self.c_frac.frombytes((taken.astype(np.float64) / np.float64(cs)).astype(np.float32).tobytes())
        self.c_gc_tot += int(taken.sum(dtype=np.int64))
        self.c_tot += cs * int(taken.shape[0])
        if stop < n:
            if n_read_level == stop:
                raise ZeroDivisionError("division by zero")
            if self.draw == "numpy":
                np.random.choice(int(lens[stop]), int(draws_per_read(lens[stop:], cs, samp_rate)[0]), replace=False)
            raise ValueError("Cannot take a larger sample than population when 'replace=False'")

    def gc_stats(self):
        """[mean, standard deviation] of the reads' GC fractions, as plot_unmasked_gc_frac returns them (lq_gcfrac.py:55)"""
        return [np.mean(self.r_frac), np.std(self.r_frac)]

    def figure_data(self, b_width=0.02, n_points=50) -> dict:
        """What plot_unmasked_gc_frac computes before it draws (lq_gcfrac.py:49-72), on the device (figdata.py): xs = np.linspace(0, 1.0,
        n_points); read_hist / chunk_hist = (edges, counts, density) of plt.hist(frac, bins=np.arange(min, max + b_width, b_width),
        density=True); read_kde / chunk_kde = gaussian_kde(frac)(xs), read_kde None for fewer than two reads as the reference skips it;
        read_bandwidth / chunk_bandwidth the standard deviations of the two Gaussians (what lq_gcfrac.py:81-84 wanted to return;
        None with read_kde); mean, sd = gc_stats().  ValueError when there is no read or no window (the reference's min() raises it),
        and when a KDE is refused (one window, or values without variance)"""
        from . import figdata
        if len(self.r_frac) == 0 or len(self.c_frac) == 0:
            raise ValueError("min() arg is an empty sequence")
        xs = np.linspace(0, 1.0, n_points)
        out = {"xs": xs}
        for key, frac in (("read", self.r_frac), ("chunk", self.c_frac)):
            a = np.array(frac, dtype=np.float32)                    # (a copy: a view would pin the array('f') against further appends)
            lo, hi = figdata.value_range(a, self.device, self.lib)
            out[key + "_hist"] = figdata.density_hist(a, float(lo), float(hi) + b_width, b_width, self.device, self.lib)
            if key == "read" and len(frac) <= 1:
                out["read_kde"] = out["read_bandwidth"] = None
                continue
            out[key + "_kde"], out[key + "_bandwidth"] = figdata.gaussian_kde_curve(a, xs, self.device, self.lib, return_bandwidth=True)
        out["mean"], out["sd"] = self.gc_stats()
        return out

    def json_block(self) -> dict:
        gc_read_mean, gc_read_sd = self.gc_stats()
        return {"GC_stats": {"Mean_GC_content": float(gc_read_mean), "SD_GC_content": float(gc_read_sd)}}

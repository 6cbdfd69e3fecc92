#!/usr/bin/env python3
"""lqchunk_sdust against lqchunk_sdust_split (the scan in pieces, kernels_dust_split.hpp) on the same resident chunk: the reads of BASELINE
configs[1] (50 000 synthetic ONT reads ~15 kb) and a slice of configs[4]'s ultra-long reads (cfg5: mean ~60 kb, N50 ~100 kb), every read
with a quality string, uploaded in mini-batches of at most --batch-mbases as lqsdust_main cuts them.  Per mini-batch the two calls are
alternated --reps times after one warm-up call of each; a repetition's time is the sum over the mini-batches (upload not counted: it is
the same for both).  Medians and the spread (min .. max), Mbases/s of the medians, the reads that took the serial walk, and whether the
two calls gave the same arrays.  --only serial|pieces: that call alone, for a `rocprofv3 --kernel-trace --stats` run around this script.
One JSON line (also written to $OUT/sdust_split_time.json when OUT is set).
Usage: python tools/sdust_split_time.py [--reads 50000] [--ultra-reads 75000] [--reps 3] [--piece 0] [--workers 16] [--only serial|pieces]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from longqc_amd import chunkpass, synth  # noqa: E402


def batches(off, cap):
    """read ranges [a, b) of at most cap bases (one read where a read alone has more)"""
    out, a = [], 0
    n = off.shape[0] - 1
    while a < n:
        b = int(np.searchsorted(off, off[a] + cap, side="right")) - 1
        b = min(max(b, a + 1), n)
        out.append((a, b))
        a = b
    return out


def time_set(label, cfg, n_reads, a):
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), n_reads=n_reads, workers=a.workers)
    flat, off = np.ascontiguousarray(F.flat), np.ascontiguousarray(F.off, dtype=np.uint64)
    n_bases = int(off[-1])
    res = {"n_reads": int(off.shape[0] - 1), "n_bases": n_bases, "setup_s": round(time.time() - t0, 1)}
    ch = chunkpass.ReadChunk(None)
    runs = {"serial": [0.0] * a.reps, "pieces": [0.0] * a.reps}
    same, n_serial, n_batches = True, 0, 0
    for lo, hi in batches(off, a.batch_mbases * 1000000):
        n = hi - lo
        seq = flat[int(off[lo]):int(off[hi])]
        qual = np.full(seq.shape[0], ord("5"), np.uint8)
        o = np.ascontiguousarray(off[lo:hi + 1] - off[lo])
        ch._ck(ch.lib.lqchunk_load(ch.h, n, seq.ctypes.data, o.ctypes.data, qual.ctypes.data))
        ch.n = n
        n_batches += 1
        out = {}
        for it in range(a.reps + 1):                                # alternated; the first call of each is the warm-up
            for mode in ("serial", "pieces"):
                if a.only and mode != a.only:
                    continue
                t = time.perf_counter()
                out[mode] = ch.sdust(split=mode, piece=a.piece or None)
                if it:
                    runs[mode][it - 1] += time.perf_counter() - t
        if not a.only:
            same = same and all(x.tobytes() == y.tobytes() for x, y in zip(out["serial"], out["pieces"]))
        if a.only != "serial":
            n_serial += ch.n_serial
    ch.close()
    res.update(mini_batches=n_batches, reads_on_the_serial_walk=n_serial, same_arrays=same if not a.only else None)
    for mode, ts in runs.items():
        if a.only and mode != a.only:
            continue
        med = statistics.median(ts)
        res[mode] = {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "mbases_per_s": round(n_bases / med / 1e6, 1)}
    if not a.only:
        res["pieces_over_serial"] = round(res["serial"]["median_s"] / res["pieces"]["median_s"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000, help="reads of configs[1] (0: skip the set)")
    ap.add_argument("--ultra-reads", type=int, default=75000, help="reads of the cfg5 slice (0: skip the set)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--piece", type=int, default=0, help="bases per piece (0: the library's default)")
    ap.add_argument("--batch-mbases", type=int, default=200)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--only", choices=("serial", "pieces"), default=None)
    a = ap.parse_args()
    res = {"metric": "seconds per pass of lqchunk_sdust / lqchunk_sdust_split over resident mini-batches (W 64, T 20)", "unit": "s", "reps": a.reps,
           "piece": a.piece or "default", "batch_mbases": a.batch_mbases, "sets": {}}
    if a.reads:
        res["sets"]["configs1_ont_15kb"] = time_set("cfg2", dataclasses.replace(synth.CONFIGS["cfg2"], nsample=10), a.reads, a)
    if a.ultra_reads:
        res["sets"]["cfg5_ultra_long"] = time_set("cfg5", synth.CONFIGS["cfg5"], a.ultra_reads, a)
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "sdust_split_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

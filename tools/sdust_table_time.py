#!/usr/bin/env python3
"""The low-complexity table of resident chunks in host mode against device mode (LqMaskMI355X(table=...)): host mode is the
scan with its arrays copied back, sdust._rows (one Python string per read) and close_pool writing them line by line; device mode is the
scan with its arrays left on the device, lqchunk_sdust_table (k_sdust_rows, k_sdust_text) and close_pool writing each chunk's bytes.  Two
sets: the reads of BASELINE configs[1] (50 000 synthetic ONT reads ~15 kb) in mini-batches of at most --batch-mbases, and a synthetic
short-read set (500 000 reads of 1 kb, one mini-batch per 100 000 reads); every read has a random quality string and a name like
m54238_180901_011437/17/ccs.  Per mini-batch (uploaded once, not timed) the two modes are alternated --reps times after one warm-up
submission of each; a repetition's time is the sum of its submit_sdust calls plus its close_pool.  Medians with the spread (min .. max),
the scan's share (ReadChunk.sdust alone, timed the same way), host_summary (the array work that host mode's submit_sdust does for summary()
and the parent commit's did not: the exclusion lists and the two sums, timed alone on the same arrays), microseconds per row of what the
modes add to the scan, and whether the two files are the same bytes.  One JSON line (also written to $OUT/sdust_table_time.json when OUT is set).
Usage: python tools/sdust_table_time.py [--reads 50000] [--short-reads 500000] [--reps 3] [--workers 16] [--split serial|pieces]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from longqc_amd import chunkpass, sdust, synth  # noqa: E402
from tools.sdust_split_time import batches  # noqa: E402

MODES = ("host", "device")


def time_set(flat, off, a, tmp, cap_bases=None, cap_reads=None):
    n_reads, n_bases = int(off.shape[0] - 1), int(off[-1])
    rng = np.random.default_rng(5)
    names = ["m54238_180901_011437/%d/ccs" % i for i in range(n_reads)]
    ranges = batches(off, cap_bases) if cap_bases else [(lo, min(lo + cap_reads, n_reads)) for lo in range(0, n_reads, cap_reads)]
    masks = {m: [sdust.LqMaskMI355X(os.path.join(tmp, "%s%d" % (m, it)), lib=None, split=a.split, table=m) for it in range(a.reps + 1)] for m in MODES}
    runs = {m: [0.0] * (a.reps + 1) for m in MODES + ("scan", "host_summary")}
    ch = chunkpass.ReadChunk(None)
    for k, (lo, hi) in enumerate(ranges):
        seq = flat[int(off[lo]):int(off[hi])]
        qual = rng.integers(35, 75, seq.shape[0], dtype=np.uint8)
        ch.load_arrays(names[lo:hi], seq, off[lo:hi + 1] - off[lo], qual)
        for it in range(a.reps + 1):                                # alternated; the first of each is the warm-up
            for m in MODES:
                t = time.perf_counter()
                masks[m][it].submit_sdust(None, k, chunk=ch)
                runs[m][it] += time.perf_counter() - t
            t = time.perf_counter()
            masked, _, qv = ch.sdust(split=a.split)
            runs["scan"][it] += time.perf_counter() - t
            t = time.perf_counter()                                 # what host mode's submit_sdust adds to the parent commit's for summary()
            sdust.exclusion_lists(masked[:ch.n], np.diff(ch.off.astype(np.int64)))
            masked[:ch.n].sum(dtype=np.uint64), qv[:ch.n].sum(dtype=np.uint64), np.array(ch.lens, dtype=np.int64)
            runs["host_summary"][it] += time.perf_counter() - t
    ch.close()
    same = True
    for it in range(a.reps + 1):
        for m in MODES:
            t = time.perf_counter()
            masks[m][it].close_pool()
            runs[m][it] += time.perf_counter() - t
        same = same and open(masks["host"][it].get_outfile_path(), "rb").read() == open(masks["device"][it].get_outfile_path(), "rb").read()
        same = same and masks["host"][it].summary() == masks["device"][it].summary()
        for m in MODES:
            os.remove(masks[m][it].get_outfile_path())
    res = {"n_reads": n_reads, "n_bases": n_bases, "mini_batches": len(ranges), "same_file_and_summary": same}
    scan = statistics.median(runs["scan"][1:])
    for m, ts in runs.items():
        ts = ts[1:]
        med = statistics.median(ts)
        res[m] = {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)}
        if m in MODES:
            res[m]["beyond_the_scan_us_per_row"] = round((med - scan) / n_reads * 1e6, 3)
    res["host_over_device"] = round(res["host"]["median_s"] / res["device"]["median_s"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000, help="reads of configs[1] (0: skip the set)")
    ap.add_argument("--short-reads", type=int, default=500000, help="reads of 1 kb (0: skip the set)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-mbases", type=int, default=200)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--split", choices=sdust.SPLIT_MODES, default="pieces")
    a = ap.parse_args()
    res = {"metric": "seconds per pass of LqMaskMI355X.submit_sdust over resident mini-batches + close_pool, table='host' against table='device'",
           "unit": "s", "reps": a.reps, "split": a.split, "sets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        if a.reads:
            cfg = dataclasses.replace(synth.CONFIGS["cfg2"], nsample=10)
            F = synth.make_reads_flat(cfg, synth.make_genome(cfg), n_reads=a.reads, workers=a.workers)
            res["sets"]["configs1_ont_15kb"] = time_set(np.ascontiguousarray(F.flat), np.ascontiguousarray(F.off, dtype=np.uint64), a, tmp,
                                                        cap_bases=a.batch_mbases * 1000000)
            del F
        if a.short_reads:
            rng = np.random.default_rng(9)
            flat = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.short_reads * 1000, dtype=np.uint8)]
            off = np.arange(a.short_reads + 1, dtype=np.uint64) * np.uint64(1000)
            res["sets"]["short_reads_1kb"] = time_set(flat, off, a, tmp, cap_reads=100000)
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "sdust_table_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

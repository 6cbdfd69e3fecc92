#!/usr/bin/env python3
"""One `calc_read_and_chunk_gc_frac` call (longqc_amd/gcfrac.py, lq_gcfrac.py:25-48) on configs[2]'s reads as one chunk: 500k
synthetic PacBio Sequel CLR reads ~10 kb (longqc_amd/synth.py) as LongQC's [name, seq] records, once per draw mode.  A call on a
small chunk first takes the device's start-up out of the figures.  Per mode: the wall of the call and its parts -- the Python
gather of the records into one buffer (and, for draw="numpy", the per-read np.random.choice calls), the C call (lqgc_reads:
upload, kernels, download) and the rest (fractions, arrays, totals) -- and Mbases/s.  Beside them, on the same host in the same
run, the reference's loop restated (per read two str.count, one np.random.choice, two str.count per accepted window) on the first
--ref-reads reads, as Mbases/s.  One JSON line (also written to $OUT/gcfrac_time.json when OUT is set).
Usage: python tools/gcfrac_time.py [--reads 500000] [--ref-reads 20000] [--workers 16]"""
import argparse
import array
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import gcfrac, synth  # noqa: E402


def reference_loop(reads, cs=150, samp_rate=0.2):
    """lq_gcfrac.py:25-48 restated -> (r_frac, c_frac, seconds inside np.random.choice)"""
    r_frac, c_frac, t_choice = array.array('f'), array.array('f'), 0.0
    for r in reads:
        s = r[1]
        l = len(s)
        r_frac.append((s.count('G') + s.count('C')) / l)
        t = time.time()
        indices = np.random.choice(l, int(float(1 / cs) * l * samp_rate), replace=False)
        t_choice += time.time() - t
        for i in indices:
            if i + cs - 1 > l:
                break
            j = i + cs
            c_frac.append(float(s.count('G', i, j) + s.count('C', i, j)) / cs)
    return r_frac, c_frac, t_choice


def timed_call(reads, draw):
    parts = {"gather_s": 0.0, "choice_s": 0.0, "c_call_s": 0.0}
    real_flatten, real_call, real_choice = gcfrac._flatten, gcfrac._call, np.random.choice

    def wrap(fn, key):
        def f(*a, **kw):
            t = time.time()
            out = fn(*a, **kw)
            parts[key] += time.time() - t
            return out
        return f
    gcfrac._flatten, gcfrac._call = wrap(real_flatten, "gather_s"), wrap(real_call, "c_call_s")
    if draw == "numpy":
        np.random.choice = wrap(real_choice, "choice_s")
    lg = gcfrac.LqGCMI355X(draw=draw, seed=1)
    try:
        t0 = time.time()
        lg.calc_read_and_chunk_gc_frac(reads)
        wall = time.time() - t0
    finally:
        gcfrac._flatten, gcfrac._call, np.random.choice = real_flatten, real_call, real_choice
    out = {"wall_s": round(wall, 3)}
    out.update({k: round(v, 3) for k, v in parts.items()})
    out["rest_s"] = round(wall - sum(parts.values()), 3)
    out["windows"] = len(lg.c_frac)
    return lg, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--ref-reads", type=int, default=20000)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    cfg = dataclasses.replace(synth.CONFIGS["cfg3"], n_reads=a.reads)
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=a.workers)
    flat = F.flat.tobytes().decode("latin-1")
    reads = [["r%07d" % i, flat[int(F.off[i]):int(F.off[i + 1])]] for i in range(len(F))]
    n_bases = F.n_bases
    del F, flat
    t_setup = time.time() - t0
    gcfrac.LqGCMI355X().calc_read_and_chunk_gc_frac(reads[:1000])                    # device start-up
    res = {"metric": "seconds per calc_read_and_chunk_gc_frac call (sampleqc GC fraction, lq_gcfrac.py:25-48)", "unit": "s",
           "n_reads": len(reads), "n_bases": n_bases, "setup_s": round(t_setup, 1)}
    for draw in ("device", "numpy"):
        lg, out = timed_call(reads, draw)
        out["mbases_per_s"] = round(n_bases / 1e6 / out["wall_s"], 1)
        res[draw] = out
        res["mean_gc_" + draw], res["sd_gc_" + draw] = (float(x) for x in lg.gc_stats())
    res["value"] = res["device"]["wall_s"]
    sub = reads[:a.ref_reads]
    sub_bases = sum(len(r[1]) for r in sub)
    t1 = time.time()
    r_frac, c_frac, t_choice = reference_loop(sub)
    t_ref = time.time() - t1
    res["reference_loop"] = {"reads": len(sub), "n_bases": sub_bases, "wall_s": round(t_ref, 3), "choice_s": round(t_choice, 3),
                             "windows": len(c_frac), "mbases_per_s": round(sub_bases / 1e6 / t_ref, 1)}
    res["speedup_device_draw"] = round(res["device"]["mbases_per_s"] / res["reference_loop"]["mbases_per_s"], 1)
    res["speedup_numpy_draw"] = round(res["numpy"]["mbases_per_s"] / res["reference_loop"]["mbases_per_s"], 1)
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "gcfrac_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

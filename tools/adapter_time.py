#!/usr/bin/env python3
"""One `cut_adapter` call (longqc_amd/adapter.py, lq_adapt.py:80-101) on configs[2]'s reads as one chunk: 500k synthetic PacBio
Sequel CLR reads ~10 kb (longqc_amd/synth.py) as LongQC's [name, seq, qual] records with '!' qualities, pb-sequel's adapter
(sampleqc.PRESET_ADAPTERS) implanted at both ends of --rate of the reads, --err substitutions / insertions / deletions
(synth's 1:6:3 mix), 0-19 bases in.  A call on a small chunk first takes the device's start-up out of the figure.  Reports the
wall of the call, the part of it spent in the C call (lqadapt_reads, windows gathered, uploaded, aligned, downloaded), the
trimmed counts and how many implants were found, as one JSON line (also written to $OUT/adapter_time.json when OUT is set).
Usage: python tools/adapter_time.py [--rate 0.3] [--err 0.1] [--reads 500000] [--workers 16]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import adapter, sampleqc, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=0.3)
    ap.add_argument("--err", type=float, default=0.1)
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    adp5, adp3 = sampleqc.PRESET_ADAPTERS["pb-sequel"]
    cfg = dataclasses.replace(synth.CONFIGS["cfg3"], n_reads=a.reads)
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=a.workers)
    rng = np.random.default_rng(29)
    mix = synth.CONFIGS["cfg3"].err_mix
    a5 = np.frombuffer(adp5.encode(), np.uint8)
    a3 = np.frombuffer(adp3.encode(), np.uint8)
    reads, n_imp = [], 0
    for i in range(len(F)):
        s = F.seq(i)
        if s.shape[0] >= 300 and rng.random() < a.rate:
            s = s.copy()
            m5 = synth._mutate(a5, rng, a.err, mix)
            m3 = synth._mutate(a3, rng, a.err, mix)
            k5, k3 = int(rng.integers(0, 20)), int(rng.integers(0, 20))
            s[k5:k5 + m5.shape[0]] = m5
            s[s.shape[0] - k3 - m3.shape[0]:s.shape[0] - k3] = m3
            n_imp += 1
        st = s.tobytes().decode("latin-1")
        reads.append(["r%07d" % i, st, "!" * len(st)])
    n_bases = F.n_bases
    del F
    t_setup = time.time() - t0
    adapter.cut_adapter([list(r) for r in reads[:1000]], adp_t=adp5, adp_b=adp3)     # device start-up
    t_c = []
    real = adapter._hits

    def timed(*args, **kw):
        t = time.time()
        out = real(*args, **kw)
        t_c.append(time.time() - t)
        return out
    adapter._hits = timed
    t1 = time.time()
    t5, t3 = adapter.cut_adapter(reads, adp_t=adp5, adp_b=adp3)
    wall = time.time() - t1
    adapter._hits = real
    res = {"metric": "seconds per cut_adapter call (sampleqc adapter search, lq_adapt.py:80-101)", "value": round(wall, 3), "unit": "s",
           "n_reads": len(reads), "n_bases": n_bases, "implanted_both_ends": n_imp, "rate": a.rate, "err": a.err,
           "c_call_s": round(t_c[0], 3), "python_s": round(wall - t_c[0], 3), "setup_s": round(t_setup, 1),
           "trimmed_5": t5[1], "trimmed_3": t3[1], "max_identity_5": t5[0], "max_identity_3": t3[0],
           "mean_pos_5": float(np.mean(t5[2])) if t5[2] else None, "mean_pos_3": float(np.mean(t3[2])) if t3[2] else None,
           "adapters": "pb-sequel (45 bp both ends)", "length": 150, "th": 0.75}
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "adapter_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

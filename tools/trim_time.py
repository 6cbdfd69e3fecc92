#!/usr/bin/env python3
"""`SampleQCPass.run_file(trim=<path>)` (longqc_amd/chunkpass.py: the trimmed reads leave the device as FASTQ text, k_fastq_format)
against the host path to the same bytes -- `run_file(trim=True)`, which brings every record to the host and trims it there, followed
by `sampleqc.write_fastq(fn, t, is_chunk=True)` for every chunk of `trimmed_chunks` -- in one process, on one synthetic FASTQ file
(--reads reads of configs[1]'s shape, longqc_amd/synth.py: 50 000 reads ~15 kb; pb-sequel's adapter at both ends of --rate of the
reads), input and outputs on tmpfs.  A run of both on the file's first 1000 reads takes the device's start-up out of the figures;
then the two paths alternate --reps times.  Reports every wall, the best of each, k_fastq_format's own time (HIP events, summed over
the run's launches) with its GB/s over 2 * kept bases + name bytes in and the text out, and whether the two files are equal, as one
JSON line (also written to $OUT/trim_time.json when OUT is set).
Usage: python tools/trim_time.py [--reads 50000] [--rate 0.3] [--reps 3] [--workers 16] [--dir /dev/shm]"""
import argparse
import dataclasses
import filecmp
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import chunkpass, sampleqc, synth  # noqa: E402

PRESET = "pb-sequel"


def write_input(path, F, rate, n=None):
    """the reads as a four-line FASTQ file with seeded qualities -> (reads, bases, name bytes)"""
    adp5, adp3 = (np.frombuffer(a.encode(), np.uint8) for a in sampleqc.PRESET_ADAPTERS[PRESET])
    rng = np.random.default_rng(29)
    n = len(F) if n is None else n
    pool = rng.integers(33, 127, 1 << 20).astype(np.uint8)
    bases = names = 0
    with open(path, "wb") as f:
        for i in range(n):
            s = F.seq(i)
            if s.shape[0] >= 300 and rng.random() < rate:
                s = s.copy()
                k5, k3 = int(rng.integers(0, 20)), int(rng.integers(0, 20))
                s[k5:k5 + adp5.shape[0]] = adp5
                s[s.shape[0] - k3 - adp3.shape[0]:s.shape[0] - k3] = adp3
            q0 = int(rng.integers(0, pool.shape[0]))
            q = np.resize(np.roll(pool, -q0), s.shape[0]) if s.shape[0] > pool.shape[0] - q0 else pool[q0:q0 + s.shape[0]]
            name = b"r%07d" % i
            f.write(b"@" + name + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
            bases += s.shape[0]; names += len(name)
    return n, bases, names


def new_path(work, path, out):
    adp5, adp3 = sampleqc.PRESET_ADAPTERS[PRESET]
    p = chunkpass.SampleQCPass(work, PRESET, adp5=adp5, adp3=adp3)
    np.random.seed(11)
    t = time.time()
    res = p.run_file(path, trim=out)
    wall = time.time() - t
    ms = p.trim_writer.kernel_ms
    p.mask.close_pool(); p.close()
    return wall, ms, res


def host_path(work, path, out):
    adp5, adp3 = sampleqc.PRESET_ADAPTERS[PRESET]
    p = chunkpass.SampleQCPass(work, PRESET, adp5=adp5, adp3=adp3)
    np.random.seed(11)
    t = time.time()
    res = p.run_file(path, trim=True)
    t_run = time.time() - t
    for ch in p.trimmed_chunks:
        sampleqc.write_fastq(out, ch, is_chunk=True)
    wall = time.time() - t
    p.trimmed_chunks = p.trimmed = None
    p.mask.close_pool(); p.close()
    return wall, t_run, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--rate", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm")
    a = ap.parse_args()
    cfg = dataclasses.replace(synth.CONFIGS["cfg2"], n_reads=a.reads)
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=a.workers)      # (forked workers: before the device is opened)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path, small = os.path.join(d, "in.fq"), os.path.join(d, "small.fq")
        n, bases, name_bytes = write_input(path, F, a.rate)
        write_input(small, F, a.rate, min(1000, n))
        del F
        t_setup = time.time() - t0
        out_new, out_host = os.path.join(d, "new.fq"), os.path.join(d, "host.fq")
        for fn, out in ((new_path, out_new), (host_path, out_host)):               # device start-up, first allocations, page cache
            fn(os.path.join(d, "w"), small, out)
            os.remove(out)
        walls_new, walls_host, runs_host, kernel_ms, equal, tuples = [], [], [], [], True, True
        for rep in range(a.reps):
            w, ms, r_new = new_path(os.path.join(d, "wn%d" % rep), path, out_new)
            walls_new.append(w); kernel_ms.append(ms)
            w, t_run, r_host = host_path(os.path.join(d, "wh%d" % rep), path, out_host)
            walls_host.append(w); runs_host.append(t_run)
            equal &= filecmp.cmp(out_new, out_host, shallow=False)
            tuples &= r_new == r_host
            text = os.path.getsize(out_new)
            os.remove(out_new); os.remove(out_host)
    kept = (text - name_bytes - 6 * n) // 2
    ms = min(kernel_ms)
    res = {"metric": "seconds per run_file(trim=<path>) against run_file(trim=True) + write_fastq (sampleqc --trim_output)", "unit": "s",
           "value": round(min(walls_new), 3), "host_path_s": round(min(walls_host), 3), "speedup": round(min(walls_host) / min(walls_new), 2),
           "walls_new_s": [round(x, 3) for x in walls_new], "walls_host_s": [round(x, 3) for x in walls_host],
           "host_run_file_s": [round(x, 3) for x in runs_host], "files_equal": bool(equal), "tuples_equal": bool(tuples),
           "n_reads": n, "n_bases": bases, "bases_kept": kept, "text_bytes": text, "name_bytes": name_bytes,
           "kernel_ms": [round(x, 3) for x in kernel_ms],
           "kernel_gb_per_s": round((2 * kept + name_bytes + text) / 1e9 / (ms / 1e3), 1) if ms > 0 else None,
           "preset": PRESET, "rate": a.rate, "dir": a.dir, "setup_s": round(t_setup, 1)}
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "trim_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0 if equal and tuples else 1


if __name__ == "__main__":
    sys.exit(main())

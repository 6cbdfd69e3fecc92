#!/usr/bin/env python3
"""The chunk loop of sampleqc plus the coverage call on configs[2]-shaped synthetic reads (longqc_amd/synth.py: PacBio Sequel CLR
~10 kb), as one chunk and as several: once through chunkpass.SampleQCPass (one gather and one upload per chunk, the packed chunks
kept on the device) and once through the separate modules as INTEGRATION.md shows them (LqMaskMI355X, cut_adapter, LqGCMI355X,
subsample_from_chunk per chunk, then sampleqc.coverage_in_memory over the chunks again).  A small chunk first takes the device's
start-up out of the figures.  Also k_chunk_pack alone: lqchunk_pack on the resident chunk, --reps calls after a warm-up, the
median wall of a call (host work list + kernel) in GB/s of its own bytes (1.375 B per base), beside a device-to-device copy of the
same number of bytes made with torch on the same device.  One JSON line (also written to $OUT/chunkpass_time.json when OUT is set).
Usage: python tools/chunkpass_time.py [--reads 500000] [--chunks 4] [--nsample 5000] [--reps 10] [--workers 16] [--only pass|separate]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from longqc_amd import adapter, chunkpass, gcfrac, sampleqc, sdust, synth  # noqa: E402

PRESET = "pb-sequel"
ADP5, ADP3 = sampleqc.PRESET_ADAPTERS[PRESET]


def cut(reads, n_chunks):
    step = (len(reads) + n_chunks - 1) // n_chunks
    return [reads[i:i + step] for i in range(0, len(reads), step)]


def run_pass(chunks, nsample, wdir):
    t0 = time.time()
    sp = chunkpass.SampleQCPass(wdir, PRESET, adp5=ADP5, adp3=ADP3, nsample=nsample)
    for c in chunks:
        sp.add_chunk(c)
    sp.mask.close_pool()
    t1 = time.time()
    text = sp.coverage()
    t2 = time.time()
    store = sp.store.nbytes
    sp.close()
    return {"loop_s": round(t1 - t0, 3), "coverage_s": round(t2 - t1, 3), "wall_s": round(t2 - t0, 3), "store_bytes": store}, text


def run_separate(chunks, nsample, wdir):
    t0 = time.time()
    lm, lg, stats = sdust.LqMaskMI355X(wdir, "sep"), gcfrac.LqGCMI355X(chunk_size=150, draw="device"), adapter.AdapterStats(ADP5, ADP3)
    s_reads, cum = [], 0
    for n, reads in enumerate(chunks):
        lm.submit_sdust(reads, n)
        stats.add(adapter.cut_adapter([list(r) for r in reads], adp_t=ADP5, adp_b=ADP3))
        s_reads = sampleqc.subsample_from_chunk(reads, cum, s_reads, nsample)
        lg.calc_read_and_chunk_gc_frac(reads)
        cum += len(reads)
    lm.close_pool()
    t1 = time.time()
    text = sampleqc.coverage_in_memory([(c, len(c), 0) for c in chunks], s_reads, preset=PRESET)
    t2 = time.time()
    return {"loop_s": round(t1 - t0, 3), "coverage_s": round(t2 - t1, 3), "wall_s": round(t2 - t0, 3)}, text


def pack_rate(reads, reps):
    import torch
    ch = chunkpass.ReadChunk(reads)
    n_bases = int(ch.lens.sum())
    ch.pack()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        ch.pack()
        ts.append(time.perf_counter() - t)
    ch.close()
    nbytes = int(n_bases * 1.375)
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")      # a copy reads and writes: the same bytes moved in all
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    cs = []
    for _ in range(reps):
        t = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        cs.append(time.perf_counter() - t)
    med, cmed = statistics.median(ts), statistics.median(cs)
    return {"n_bases": n_bases, "bytes": nbytes, "reps": reps, "call_ms_median": round(med * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3),
            "call_gb_per_s": round(nbytes / med / 1e9, 1), "copy_ms_median": round(cmed * 1e3, 3), "copy_gb_per_s": round(nbytes / cmed / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--nsample", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--only", choices=("pass", "separate"), default=None)
    a = ap.parse_args()
    cfg = dataclasses.replace(synth.CONFIGS["cfg3"], n_reads=a.reads)
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=a.workers)
    flat = F.flat.tobytes().decode("latin-1")
    reads = [["r%07d" % i, flat[int(F.off[i]):int(F.off[i + 1])], "5" * int(F.off[i + 1] - F.off[i])] for i in range(len(F))]
    n_bases = F.n_bases
    del F, flat
    res = {"metric": "seconds for sampleqc's chunk loop plus the coverage call", "unit": "s", "n_reads": len(reads), "n_bases": n_bases,
           "nsample": a.nsample, "setup_s": round(time.time() - t0, 1)}
    with tempfile.TemporaryDirectory() as d:
        run_pass([reads[:1000]], 100, d)                            # device start-up
        texts = {}
        for label, chunks in (("one_chunk", [reads]), ("%d_chunks" % a.chunks, cut(reads, a.chunks))):
            out = {}
            if a.only != "separate":
                out["pass"], texts[label, "pass"] = run_pass(chunks, a.nsample, d)
            if a.only != "pass":
                out["separate"], texts[label, "separate"] = run_separate(chunks, a.nsample, d)
            if len(out) == 2:
                out["same_table"] = texts[label, "pass"] == texts[label, "separate"]
                out["speedup"] = round(out["separate"]["wall_s"] / out["pass"]["wall_s"], 2)
            res[label] = out
    if a.only != "separate":
        res["k_chunk_pack"] = pack_rate(reads, a.reps)
        res["value"] = res["one_chunk"]["pass"]["wall_s"]
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "chunkpass_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

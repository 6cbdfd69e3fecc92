#!/usr/bin/env python3
"""File to resident chunks for an unaligned BAM, on configs[2]-shaped synthetic reads (longqc_amd/synth.py: PacBio Sequel CLR ~10 kb):
the bare chunkpass.FileChunks loop (chunk_size 0.5 GiB) over
  bam        the reads written by tests/bam_writer.py (level 6, 65 280-byte payloads, no qualities, no tags), 16 inflate threads and 1;
  bam_tags   the same with two 1-B-per-base tag arrays per read (B:C, the size of PacBio kinetics), 16 threads;
  fastq_gz   the same reads as a one-line FASTQ, gzip level 6 -- what a BAM user had to convert to before: the reference point (the
             FASTA/FASTQ path does not change with the BAM reader, so this is the earlier loop).
--reps repetitions each after one warm-up pass, the median and the spread (min .. max), seconds per Gbase.  The BAM loop at 16 threads
must be faster per base than the reference point outside the spread (max < min): exit code 1 otherwise.
--only bam: the BAM loop alone, for a `rocprofv3 --kernel-trace --stats` run around this script (k_bam_gather's time comes from its
statistics; it moves 1.5 B per base).  One JSON line (also written to $OUT/bam_time.json when OUT is set).
--inflate host,device (or one of them): the inflate modes of FileChunks side by side instead -- the BAM at 16 threads and the same
reads as a bgzip FASTQ (BGZF blocks of 65 280 bytes; "host" is gzread's one thread for it), the modes alternated within every
repetition, the median and the spread per mode; $OUT/bam_time_inflate.json.  Around a `rocprofv3 --kernel-trace --stats` run with
--inflate device, k_bgzf_inflate's time per launch comes from the statistics.
--walk host,device and --host-copy all,needed (with --inflate): FileChunks' bam_walk and host_copy modes as well -- every combination
of the three lists is a mode of its own ("device/device/needed": inflate, walk, host copy), alternated within every repetition on
the BAM and on the tagged BAM (the bgzip FASTQ is left out: it has no record walk); both are meaningful with --inflate device.
Usage: python tools/bam_time.py [--reads 500000] [--chunk-mb 512] [--reps 3] [--workers 16] [--only bam] [--inflate host,device]
       [--walk host,device] [--host-copy all,needed]"""
import argparse
import dataclasses
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import chunkpass, synth  # noqa: E402
from tests import bam_writer as BW  # noqa: E402


def bam_stream(F, with_tags):
    """bam_writer's layout with numpy doing the packing: -> the inflated bytes"""
    code = np.zeros(256, np.uint8)
    code[list(BW.CODES)] = np.arange(16)
    parts = [BW.header()]
    for i in range(len(F)):
        s = code[F.seq(i)]
        l = s.shape[0]
        if l & 1:
            s = np.append(s, np.uint8(0))
        name = b"r%07d\0" % i
        tags = b""
        if with_tags:
            arr = struct.pack("<cI", b"C", l) + bytes(l)
            tags = b"ipB" + arr + b"pwB" + arr
        body = (struct.pack("<iiBBHHHIiii", -1, -1, len(name), 0, 4680, 0, 4, l, -1, -1, 0) + name + (s[0::2] << 4 | s[1::2]).tobytes()
                + b"\xff" * l + tags)
        parts.append(struct.pack("<i", len(body)) + body)
    return b"".join(parts)


def write_bgzf(path, stream, pool):
    view = memoryview(stream)
    with open(path, "wb") as f:
        for blk in pool.map(lambda i: BW.bgzf_block(bytes(view[i:i + 65280]), 6), range(0, len(stream), 65280)):
            f.write(blk)
        f.write(BW.EOF_BLOCK)


def write_fastq_gz(path, F, pool):
    """a gzip file of members of 32 MiB of text (members only so that 16 threads can write it; gzread inflates them in turn)"""
    flat, off = F.flat.tobytes(), F.off
    text = b"".join(b"@r%07d\n%s\n+\n%s\n" % (i, flat[int(off[i]):int(off[i + 1])], b"!" * int(off[i + 1] - off[i])) for i in range(len(F)))

    def member(i):
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        return c.compress(text[i:i + (32 << 20)]) + c.flush()
    with open(path, "wb") as f:
        for m in pool.map(member, range(0, len(text), 32 << 20)):
            f.write(m)
    return len(text)


def one_pass(path, cs, threads, inflate=None, walk=None, host_copy=None):
    t = time.perf_counter()
    n, nb = 0, 0
    for ch, _n_seqs, nb in chunkpass.FileChunks(path, chunk_size=cs, n_threads=threads, inflate=inflate, bam_walk=walk, host_copy=host_copy):
        n += ch.n
    return n, nb, time.perf_counter() - t


def loop(path, cs, threads, reps):
    ts, n, nb = [], 0, 0
    for _ in range(reps + 1):
        n, nb, t = one_pass(path, cs, threads)
        ts.append(t)
    return n, nb, ts[1:]


def inflate_modes(a, F, cs, res, d, pool):
    """--inflate: the modes alternated on the BAM and on the bgzip FASTQ of the same reads"""
    modes = a.inflate.split(",")
    n_reads, n_bases = len(F), int(F.n_bases)
    bam, fq = os.path.join(d, "all.bam"), os.path.join(d, "all.fastq.gz")
    stream = bam_stream(F, False)
    write_bgzf(bam, stream, pool)
    res["bam_bytes"], res["bam_inflated_bytes"] = os.path.getsize(bam), len(stream)
    flat, off = F.flat.tobytes(), F.off
    stream = b"".join(b"@r%07d\n%s\n+\n%s\n" % (i, flat[int(off[i]):int(off[i + 1])], b"!" * int(off[i + 1] - off[i])) for i in range(n_reads))
    write_bgzf(fq, stream, pool)
    res["fastq_bgzf_bytes"], res["fastq_bytes"] = os.path.getsize(fq), len(stream)
    del stream, flat
    for key, path in (("bam_16_threads", bam), ("fastq_bgzf", fq)):
        ts = {m: [] for m in modes}
        for rep in range(a.reps + 1):                               # (the first pass of every mode is the warm-up)
            for m in modes:
                n, nb, t = one_pass(path, cs, 16, m)
                assert (n, nb) == (n_reads, n_bases), (key, m, n, nb)
                if rep:
                    ts[m].append(t)
        for m in modes:
            res["%s_%s" % (key, m)] = dict(summary(ts[m], n_bases), runs_s=[round(t, 4) for t in ts[m]])
    if len(modes) == 2:
        for key in ("bam_16_threads", "fastq_bgzf"):
            res["%s_%s_over_%s" % (key, modes[0], modes[1])] = round(res["%s_%s" % (key, modes[0])]["median_s"] / res["%s_%s" % (key, modes[1])]["median_s"], 2)
    res["value"] = res["bam_16_threads_%s" % modes[-1]]["median_s"]


def walk_modes(a, F, cs, res, d, pool):
    """--walk / --host-copy: every (inflate, walk, host copy) alternated on the BAM and on the tagged BAM"""
    modes = [(i, w, h) for i in a.inflate.split(",") for w in a.walk.split(",") for h in a.host_copy.split(",")]
    n_reads, n_bases = len(F), int(F.n_bases)
    for key, tags in (("bam_16_threads", False), ("bam_tags_16_threads", True)):
        path = os.path.join(d, key + ".bam")
        stream = bam_stream(F, tags)
        write_bgzf(path, stream, pool)
        res[key + "_bytes"], res[key + "_inflated_bytes"] = os.path.getsize(path), len(stream)
        del stream
        ts = {m: [] for m in modes}
        for rep in range(a.reps + 1):                               # (the first pass of every mode is the warm-up)
            for m in modes:
                n, nb, t = one_pass(path, cs, 16, *m)
                assert (n, nb) == (n_reads, n_bases), (key, m, n, nb)
                if rep:
                    ts[m].append(t)
        for m in modes:
            res["%s_%s" % (key, "/".join(m))] = dict(summary(ts[m], n_bases), runs_s=[round(t, 4) for t in ts[m]])
    res["value"] = res["bam_16_threads_%s" % "/".join(modes[-1])]["median_s"]


def summary(ts, n_bases):
    med = statistics.median(ts)
    return {"median_s": round(med, 3), "min_s": round(min(ts), 3), "max_s": round(max(ts), 3), "s_per_gbase": round(med / n_bases * 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--chunk-mb", type=float, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--only", choices=("bam",), default=None)
    ap.add_argument("--inflate", default=None, help="host, device or host,device: compare FileChunks' inflate modes instead")
    ap.add_argument("--walk", default=None, help="host, device or host,device: FileChunks' bam_walk modes (with --inflate)")
    ap.add_argument("--host-copy", default=None, help="all, needed or all,needed: FileChunks' host_copy modes (with --inflate)")
    a = ap.parse_args()
    if a.inflate and not set(a.inflate.split(",")) <= {"host", "device"}:
        ap.error("--inflate takes host, device or host,device")
    if (a.walk or a.host_copy) and not a.inflate:
        ap.error("--walk and --host-copy go with --inflate")
    if (a.walk and not set(a.walk.split(",")) <= {"host", "device"}) or (a.host_copy and not set(a.host_copy.split(",")) <= {"all", "needed"}):
        ap.error("--walk takes host,device and --host-copy all,needed")
    cfg = dataclasses.replace(synth.CONFIGS["cfg3"], n_reads=a.reads)
    cs = int(a.chunk_mb * 1024 ** 2)
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=a.workers)
    n_reads, n_bases = len(F), int(F.n_bases)
    res = {"metric": "seconds from the file to resident chunks (bare FileChunks loop)", "unit": "s", "n_reads": n_reads, "n_bases": n_bases,
           "chunk_size": cs, "reps": a.reps}
    ok = True
    if a.inflate:
        with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(a.workers) as pool:
            if a.walk or a.host_copy:
                a.walk, a.host_copy = a.walk or "host", a.host_copy or "all"
                walk_modes(a, F, cs, res, d, pool)
            else:
                inflate_modes(a, F, cs, res, d, pool)
        res["setup_and_run_s"] = round(time.time() - t0, 1)
        print(json.dumps(res))
        if os.environ.get("OUT"):
            os.makedirs(os.environ["OUT"], exist_ok=True)
            with open(os.path.join(os.environ["OUT"], "bam_time_walk.json" if a.walk else "bam_time_inflate.json"), "w") as f:
                f.write(json.dumps(res) + "\n")
        return 0
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(a.workers) as pool:
        bam = os.path.join(d, "all.bam")
        stream = bam_stream(F, False)
        write_bgzf(bam, stream, pool)
        res["bam_bytes"], res["bam_inflated_bytes"] = os.path.getsize(bam), len(stream)
        del stream
        if a.only is None:
            tagged, fq = os.path.join(d, "tags.bam"), os.path.join(d, "all.fastq.gz")
            stream = bam_stream(F, True)
            write_bgzf(tagged, stream, pool)
            res["bam_tags_bytes"], res["bam_tags_inflated_bytes"] = os.path.getsize(tagged), len(stream)
            del stream
            res["fastq_bytes"], res["fastq_gz_bytes"] = write_fastq_gz(fq, F, pool), os.path.getsize(fq)
        del F
        res["setup_s"] = round(time.time() - t0, 1)
        for key, path, threads in (("bam_16_threads", bam, 16), ("bam_1_thread", bam, 1)) + (
                (("bam_tags_16_threads", tagged, 16), ("fastq_gz", fq, 16)) if a.only is None else ()):
            n, nb, ts = loop(path, cs, threads, a.reps)
            assert (n, nb) == (n_reads, n_bases), (key, n, nb)
            res[key] = summary(ts, n_bases)
            if key == "bam_1_thread" and a.only:
                break
        if a.only is None:
            ok = res["bam_16_threads"]["max_s"] < res["fastq_gz"]["min_s"]
            res["bam_faster_than_fastq_gz_outside_the_spread"] = ok
            res["fastq_gz_over_bam"] = round(res["fastq_gz"]["median_s"] / res["bam_16_threads"]["median_s"], 2)
        res["value"] = res["bam_16_threads"]["median_s"]
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "bam_time.json" if a.only is None else "bam_time_only_bam.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

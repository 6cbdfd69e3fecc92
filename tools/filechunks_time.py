#!/usr/bin/env python3
"""File to finished chunk loop, on configs[2]-shaped synthetic reads (longqc_amd/synth.py: PacBio Sequel CLR ~10 kb) written as a
one-line FASTQ: (a) chunkpass.SampleQCPass.run_file(path) -- the file read, parsed and gathered by the library (lqreader_*,
k_chunk_gather) -- against the add_chunk(reads) loop fed by a pure-Python reader (the file's lines in strides of four: nothing faster
exists in Python for a one-line FASTQ), the reader's time reported apart; --reps alternated repetitions, medians and the spread
(min .. max).  Both loops cut the chunks at the same borders and must leave the same sdust table and subsample.
(b) --only gather: FileChunks alone, --reps times over the file, for a `rocprofv3 --kernel-trace --stats` run around this script
(k_chunk_gather's time comes from its statistics), and a device-to-device copy of the bytes the two launches move (torch, same
process, wall time of copy + synchronize; under rocprofv3 its kernel is in the same statistics).  One JSON line (also written to $OUT/filechunks_time.json when OUT is set).
(c) --inflate host,device: the same FASTQ as a plain .gz (zlib level 6, one member), FileChunks alone in each mode named -- gzread
on one thread against the speculative spans of csrc/gzip.hpp -- alternated, one warm-up pass and --reps timed ones per mode, medians
and the spread, the device mode's inflate_stats; the modes must count the same reads and bases.
(d) --parse host,device: the record scan on the device (lqreader_parse, k_fx_*) against the host parser, alternated, one warm-up pass
and --reps timed ones per mode, medians and the spread: the bare FileChunks loop and run_file on the one-line FASTQ, the bare loop on
the same reads as FASTA wrapped at 60 columns and on the FASTQ as level-6 gzip with inflate="device"; parse_stats of the device mode.
(e) --inflate device --parse device --host-copy all,needed: the FASTQ as bgzip (64-KiB members, level 6) and as one level-6 gzip
member, the bare FileChunks loop with the inflated bytes copied back ("all", the path of (c) and (d)) and left on the device
("needed": k_crc32_ranges, k_fx_names), alternated, one warm-up pass and --reps timed ones per mode, medians and the spread, copy_stats,
parse_stats and inflate_stats of each; beside them the host default (inflate="host", parse="host") on the same files.
Usage: python tools/filechunks_time.py [--reads 500000] [--chunk-mb 512] [--nsample 5000] [--reps 3] [--workers 16] [--only loop|gather]
       python tools/filechunks_time.py --reads 50000 --inflate host,device [--reps 3]
       python tools/filechunks_time.py --reads 50000 --parse host,device [--reps 3]
       python tools/filechunks_time.py --reads 50000 --inflate device --parse device --host-copy all,needed [--reps 3]"""
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

from longqc_amd import chunkpass, sampleqc, synth  # noqa: E402

PRESET = "pb-sequel"
ADP5, ADP3 = sampleqc.PRESET_ADAPTERS[PRESET]


def python_chunks(path, cs):
    """lq_utils.parse_fastx_chunk for a one-line FASTQ without pysam: -> the chunks as lists of [name, seq, qual]"""
    ov = sys.getsizeof("")
    with open(path) as f:
        lines = f.read().split("\n")
    out, cur, size = [], [], 0
    for i in range(0, len(lines) - 3, 4):
        name, seq, qual = lines[i][1:].split(None, 1)[0], lines[i + 1].upper(), lines[i + 3]
        cur.append([name, seq, qual])
        size += 3 * ov + len(name) + len(seq) + len(qual)
        if size >= cs:
            out.append(cur)
            size, cur = 0, []
    out.append(cur)
    return out


def new_loop(path, cs, nsample, wdir):
    t0 = time.time()
    sp = chunkpass.SampleQCPass(wdir, PRESET, adp5=ADP5, adp3=ADP3, nsample=nsample, suffix="new")
    sp.run_file(path, chunk_size=cs)
    sp.mask.close_pool()
    t1 = time.time()
    out = (open(sp.mask.get_outfile_path()).read(), sp.s_reads, sp.chunk_n)
    sp.close()
    return {"wall_s": t1 - t0}, out


def old_loop(path, cs, nsample, wdir):
    t0 = time.time()
    chunks = python_chunks(path, cs)
    t1 = time.time()
    sp = chunkpass.SampleQCPass(wdir, PRESET, adp5=ADP5, adp3=ADP3, nsample=nsample, suffix="old")
    for c in chunks:
        sp.add_chunk(c)
    sp.mask.close_pool()
    t2 = time.time()
    out = (open(sp.mask.get_outfile_path()).read(), sp.s_reads, sp.chunk_n)
    sp.close()
    return {"reader_s": t1 - t0, "loop_s": t2 - t1, "wall_s": t2 - t0}, out


def summary(runs):
    return {k: {"median": round(statistics.median(r[k] for r in runs), 3), "min": round(min(r[k] for r in runs), 3),
                "max": round(max(r[k] for r in runs), 3)} for k in runs[0]}


def gather_only(path, cs, reps, n_bases):
    import torch
    ts = []
    for _ in range(reps + 1):
        t = time.perf_counter()
        n = sum(ch.n for ch, _, _ in chunkpass.FileChunks(path, chunk_size=cs))
        ts.append(time.perf_counter() - t)
    a = torch.empty(2 * n_bases, dtype=torch.uint8, device="cuda")     # the two launches read and write n_bases each: a copy of 2 n_bases moves as much
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(reps, 5)):
        t = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    med = statistics.median(ms)
    return {"reads": n, "file_to_chunks_s": [round(x, 3) for x in ts[1:]], "file_to_chunks_first_s": round(ts[0], 3), "bytes_moved": 4 * n_bases,
            "copy_ms_median": round(med, 3), "copy_ms_min": round(min(ms), 3), "copy_gb_per_s": round(4 * n_bases / med / 1e6, 1)}


def inflate_modes(path, cs, reps, modes):
    import zlib
    gz = path + ".gz"
    t0 = time.time()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "rb") as f, open(gz, "wb") as g:
        for block in iter(lambda: f.read(1 << 24), b""):
            g.write(c.compress(block))
        g.write(c.flush())
    out = {"gz_bytes": os.path.getsize(gz), "compress_s": round(time.time() - t0, 1), "modes": {}}
    runs, counts, stats = {m: [] for m in modes}, {}, {}
    for it in range(reps + 1):                                  # alternated; the first pass of every mode is the warm-up
        for m in modes:
            fc = chunkpass.FileChunks(gz, chunk_size=cs, inflate=m)
            t = time.perf_counter()
            tot = [(ns, nb) for _, ns, nb in fc][-1]
            if it:
                runs[m].append({"wall_s": time.perf_counter() - t})
            counts[m], stats[m] = tot, fc.inflate_stats
    for m in modes:
        out["modes"][m] = dict(summary(runs[m]), reads_bases=counts[m], inflate_stats=stats[m])
    out["same_counts"] = len(set(counts.values())) == 1
    return out


def parse_modes(path, cs, reps, modes, nsample, wdir):
    import zlib
    fa, gz = path[:-3] + ".fa", path + ".gz"
    with open(path, "rb") as f, open(fa, "wb") as g:               # the same reads as FASTA wrapped at 60 columns
        lines = f.read().split(b"\n")
        for i in range(0, len(lines) - 3, 4):
            s = lines[i + 1]
            g.write(b">" + lines[i][1:] + b"\n" + b"".join(s[k:k + 60] + b"\n" for k in range(0, len(s), 60)))
        del lines
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "rb") as f, open(gz, "wb") as g:
        for block in iter(lambda: f.read(1 << 24), b""):
            g.write(c.compress(block))
        g.write(c.flush())
    out = {}
    cases = (("fastq", path, {}), ("fasta_w60", fa, {}), ("fastq_gz_inflate_device", gz, {"inflate": "device"}))
    for label, p, kw in cases:
        runs, counts, stats = {m: [] for m in modes}, {}, {}
        for it in range(reps + 1):                                  # alternated; the first pass of every mode is the warm-up
            for m in modes:
                fc = chunkpass.FileChunks(p, chunk_size=cs, parse=m, **kw)
                t = time.perf_counter()
                tot = [(ns, nb) for _, ns, nb in fc][-1]
                if it:
                    runs[m].append({"wall_s": time.perf_counter() - t})
                counts[m], stats[m] = tot, fc.parse_stats
        out[label] = {"file_bytes": os.path.getsize(p), "same_counts": len(set(counts.values())) == 1,
                      "modes": {m: dict(summary(runs[m]), reads_bases=counts[m], parse_stats=stats[m]) for m in modes}}
    runs, outs = {m: [] for m in modes}, {}
    for it in range(reps + 1):
        for m in modes:
            t = time.perf_counter()
            sp = chunkpass.SampleQCPass(wdir, PRESET, adp5=ADP5, adp3=ADP3, nsample=nsample, suffix=m)
            sp.run_file(path, chunk_size=cs, parse=m)
            sp.mask.close_pool()
            if it:
                runs[m].append({"wall_s": time.perf_counter() - t})
            outs[m] = (open(sp.mask.get_outfile_path()).read(), sp.s_reads, sp.chunk_n)
            sp.close()
    out["run_file_fastq"] = {"same_results": len({repr(v) for v in outs.values()}) == 1, "modes": {m: summary(runs[m]) for m in modes}}
    return out


def hostcopy_modes(path, cs, reps, modes, inflate, parse):
    import zlib
    from tests import bam_writer
    bg, gz = path + ".bgz.gz", path + ".gz"
    t0 = time.time()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "rb") as f, open(gz, "wb") as g, open(bg, "wb") as b:
        for block in iter(lambda: f.read(65280 * 256), b""):
            g.write(c.compress(block))
            b.write(bam_writer.bgzf(block, eof=False))
        g.write(c.flush())
        b.write(bam_writer.bgzf(b""))
    out = {"compress_s": round(time.time() - t0, 1), "inflate": inflate, "parse": parse}
    for label, p in (("fastq_bgzip", bg), ("fastq_gzip", gz)):
        cases = [("host_copy=" + m, dict(inflate=inflate, parse=parse, host_copy=m)) for m in modes] + [("host_default", dict(inflate="host", parse="host"))]
        runs, counts, stats = {k: [] for k, _ in cases}, {}, {}
        for it in range(reps + 1):                                  # alternated; the first pass of every mode is the warm-up
            for k, kw in cases:
                fc = chunkpass.FileChunks(p, chunk_size=cs, **kw)
                t = time.perf_counter()
                tot = [(ns, nb) for _, ns, nb in fc][-1]
                if it:
                    runs[k].append({"wall_s": time.perf_counter() - t})
                counts[k], stats[k] = tot, dict(copy_stats=fc.copy_stats, parse_stats=fc.parse_stats, inflate_stats=fc.inflate_stats)
        out[label] = {"file_bytes": os.path.getsize(p), "same_counts": len(set(counts.values())) == 1,
                      "modes": {k: dict(summary(runs[k]), reads_bases=counts[k], **stats[k]) for k, _ in cases}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--chunk-mb", type=float, default=512)
    ap.add_argument("--nsample", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--only", choices=("loop", "gather"), default=None)
    ap.add_argument("--inflate", default=None, help="host,device: time FileChunks on the file as a plain .gz in these modes, and nothing else")
    ap.add_argument("--parse", default=None, help="host,device: time FileChunks and run_file with the record scan in these modes, and nothing else")
    ap.add_argument("--host-copy", default=None, help="all,needed: with --inflate device --parse device, time FileChunks on the file as bgzip and as gzip in these modes, and nothing else")
    a = ap.parse_args()
    cfg = dataclasses.replace(synth.CONFIGS["cfg3"], n_reads=a.reads)
    cs = int(a.chunk_mb * 1024 ** 2)
    t0 = time.time()
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=a.workers)
    flat, off, n_bases = F.flat.tobytes(), F.off, int(F.n_bases)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "all.fq")
        with open(path, "wb") as f:
            for i in range(len(F)):
                s = flat[int(off[i]):int(off[i + 1])]
                f.write(b"@r%07d\n%s\n+\n%s\n" % (i, s, b"5" * len(s)))
        res = {"metric": "seconds from the FASTQ file to the finished chunk loop", "unit": "s", "n_reads": len(F), "n_bases": n_bases,
               "file_bytes": os.path.getsize(path), "chunk_size": cs, "nsample": a.nsample, "setup_s": round(time.time() - t0, 1)}
        del F, flat
        sum(ch.n for ch, _, _ in chunkpass.FileChunks(path, chunk_size=cs))       # device start-up, the file in the page cache
        if a.host_copy:
            res["metric"] = "seconds from the bgzip / gzip FASTQ file to its chunks on the device, by host_copy mode"
            res["host_copy"] = hostcopy_modes(path, cs, a.reps, a.host_copy.split(","), a.inflate or "device", a.parse or "device")
        elif a.inflate:
            res["metric"] = "seconds from the gzip FASTQ file to its chunks on the device"
            res["inflate"] = inflate_modes(path, cs, a.reps, a.inflate.split(","))
        elif a.parse:
            res["metric"] = "seconds from the file to its chunks on the device, by parse mode"
            res["parse"] = parse_modes(path, cs, a.reps, a.parse.split(","), a.nsample, d)
        elif a.only != "gather":
            news, olds, same = [], [], True
            for _ in range(a.reps):                                 # alternated
                r_new, o_new = new_loop(path, cs, a.nsample, d)
                r_old, o_old = old_loop(path, cs, a.nsample, d)
                news.append(r_new); olds.append(r_old)
                same = same and o_new == o_old
            res.update(run_file=summary(news), python_reader_and_add_chunk=summary(olds), same_results=same, reps=a.reps, chunks=o_new[2])
            res["value"] = res["run_file"]["wall_s"]["median"]
        if a.only != "loop" and not a.inflate and not a.parse and not a.host_copy:
            res["gather"] = gather_only(path, cs, a.reps, n_bases)
    print(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "filechunks_time.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

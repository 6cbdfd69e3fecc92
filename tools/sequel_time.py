#!/usr/bin/env python3
"""The Sequel platform QC (longqc_amd/sequel.py) on a synthetic run: N ZMWs of 2..40 touching items (subreads with adapters between
them, an LQ stretch at either end, the odd gap, a control read now and then); every record has 300 bases and the tags a Sequel file
carries (RG, sn, an ip array as long as the read); written in tests/bam_writer.py's layout at zlib level 1.  Timed, after a start-up call
on a small run: file -> JSON block and figure data for each byte path (host inflate; device inflate; device inflate with the bytes kept
on the device), and lqpol_add_bytes (pieces of 64 MB) + lqpol_finish from inflated bytes in memory.  The kernels alone: a child process
of this tool runs the same bytes once more (after a first pass for the buffers) with LQCOV_TIMING=1, under which the library closes every
stage with a wait and prints its time: the record walk, k_pol_fields + k_pol_compact, and lqpol_finish's three stages
("kernel_stages_ms"; the waits slow the call, so these come from that run of their own).  Beside it, alternated in the same run on
the same host, the plain Python model of the reference's loop (set_scrap / set_subreads / construct_polread restated over (name, sz, sc) tuples already in memory: the pysam iteration
the reference pays on top is not in it).  The two sides' per-ZMW integers must be equal.  Median (min-max) seconds over --reps; one JSON
line per size, also written to $OUT/sequel_time.json when OUT is set.
Usage: python tools/sequel_time.py [--zmws 20000,100000] [--reps 3]"""
import argparse
import json
import os
import statistics
import re
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import sequel  # noqa: E402
from tests import bam_writer as BW  # noqa: E402
from tests.test_polread_walk import model  # noqa: E402

HEADER = "@HD\tVN:1.5\tSO:unknown\n@RG\tID:a1b2c3d4\tPL:PACBIO\tDS:READTYPE=%s;BINDINGKIT=100\tPU:m54_1\n"
READ_LEN = 300
PATHS = (("host", "all"), ("device", "all"), ("device", "needed"))


def make_run(n_zmw, seed):
    """-> (scraps [(name, sz, sc)], subreads [name]) in file order: ZMW after ZMW, as a Sequel file has them"""
    rng = np.random.default_rng(seed)
    scraps, subreads = [], []
    for z, n in zip(rng.choice(n_zmw * 8, n_zmw, replace=False).tolist(), rng.integers(2, 41, n_zmw).tolist()):
        pos, lens = 0, rng.integers(30, 9000, n).tolist()
        for k in range(n):
            ln = lens[k] if k % 2 == 0 else 45
            cls = "L" if k in (0, n - 1) and n > 2 else "SA"[k % 2]
            pos += 17 if k and k % 11 == 0 else 0
            name = "m54_1/%d/%d_%d" % (z, pos, pos + ln)
            if cls == "S":
                subreads.append(name)
            else:
                scraps.append((name, "N", cls))
            pos += ln
        if z % 13 == 0:
            scraps.append(("m54_1/%d/0_%d" % (z, lens[0]), "C", "F"))
    return scraps, subreads


def write_files(d, scraps, subreads):
    """-> the two inflated streams (bam_writer.record's layout, the parts every record shares made once)"""
    tail = BW.pack_seq((b"ACGT" * READ_LEN)[:READ_LEN]) + b"\xff" * READ_LEN
    shared = b"RGZa1b2c3d4\0" + b"snBf" + struct.pack("<I4f", 4, 7.5, 8.25, 9.0, 10.5) + b"ipBC" + struct.pack("<I", READ_LEN) + bytes(READ_LEN)

    def record(name, tags):
        nm = name.encode() + b"\0"
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm), 0, 4680, 0, 4, READ_LEN, -1, -1, 0) + nm + tail + tags + shared
        return struct.pack("<i", len(body)) + body

    streams = []
    for fname, rt, recs in (("m54_1.scraps.bam", "SCRAP", [record(n, ("szA%sscA%s" % (sz, sc)).encode()) for n, sz, sc in scraps]),
                            ("m54_1.subreads.bam", "SUBREAD", [record(n, b"") for n in subreads])):
        streams.append(BW.header((HEADER % rt).encode()) + b"".join(recs))
        with open(os.path.join(d, fname), "wb") as f:
            f.write(BW.bgzf(streams[-1], level=1))
    return streams


def python_model(scraps, subreads):
    """lq_sequel.py:25-73 and 284-296 over tuples in memory -> ({zmw: (hq, tot, is_pol, ad_num)}, control)"""
    reads, control = {}, 0
    for name, sz, sc in scraps + [(n, "N", "S") for n in subreads]:
        f = name.split("/")
        p = f[2].split("_")
        if sz == "N":
            reads.setdefault(f[1], []).append((int(p[0]), int(p[1]), sc))
        elif sz == "C" and sc == "F":
            control += int(p[1]) - int(p[0]) + 1
    return {int(z): model(items) for z, items in reads.items()}, control


def spread(vals):
    return "%.4f (%.4f-%.4f)" % (statistics.median(vals), min(vals), max(vals))


def from_bytes(streams, piece=64 << 20):
    """lqpol_add_bytes over both files' inflated bytes, then lqpol_finish -> (seconds of each, the finished handle)"""
    p = sequel.PolymeraseReads()
    t0 = time.perf_counter()
    for kind, data in enumerate(streams):
        at = len(BW.header((HEADER % ("SCRAP", "SUBREAD")[kind]).encode()))
        while at < len(data):
            at += p.add_bytes(kind, data[at:at + piece], 0)
    t1 = time.perf_counter()
    p.finish()
    return t1 - t0, time.perf_counter() - t1, p


def kernel_stages(n_zmw):
    """-> {stage: ms} from a child's second pass over the same bytes, printed by the library under LQCOV_TIMING"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-child", str(n_zmw)], env=dict(os.environ, LQCOV_TIMING="1"),
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rec, fin = ([l for l in r.stderr.splitlines() if l.startswith(k)][-1] for k in ("lqpol records", "lqpol_finish"))
    out = {}
    for line in (rec, fin):                                          # "<what>: <counts>: <stage> <ms> <stage> <ms> .. ms"
        for name, ms in re.findall(r"([A-Za-z_+/0-9 ]+?) ([0-9.]+)(?= |$)", line.split(": ", 2)[2].replace(" ms", "")):
            out[name.strip()] = float(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", default="20000,100000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages-child", type=int, default=0, help="(the tool's own child: two passes of lqpol_add_bytes + lqpol_finish over a run of that many ZMWs)")
    a = ap.parse_args()
    if a.stages_child:
        with tempfile.TemporaryDirectory() as d:
            streams = write_files(d, *make_run(a.stages_child, 100 + a.stages_child))
            for _ in range(2):
                from_bytes(streams)[2].close()
        return
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for n_zmw in [300] + [int(x) for x in a.zmws.split(",")]:      # (the first, small run: device start-up, not reported)
            run = os.path.join(d, "run%d" % n_zmw)
            os.makedirs(run)
            scraps, subreads = make_run(n_zmw, 100 + n_zmw)
            streams = write_files(run, scraps, subreads)
            t = {"file_to_json_%s_inflate_%s_s" % k: [] for k in PATHS}
            t.update(add_bytes_s=[], finish_s=[], python_model_s=[])
            for _ in range(a.reps):
                for inflate, host_copy in PATHS:
                    t0 = time.perf_counter()
                    js, fig = sequel.run_platformqc(run, inflate=inflate, host_copy=host_copy)
                    t["file_to_json_%s_inflate_%s_s" % (inflate, host_copy)].append(time.perf_counter() - t0)
                ta, tf, p = from_bytes(streams)
                t["add_bytes_s"].append(ta); t["finish_s"].append(tf)
                t0 = time.perf_counter()
                want, control = python_model(scraps, subreads)
                t["python_model_s"].append(time.perf_counter() - t0)
                got = {int(z): (int(h), int(q), bool(i), int(n)) for z, h, q, i, n in zip(p.all_zmw, p.all_hq, p.all_tot, p.is_pol, p.all_ad_num)}
                assert got == want and p.control_throughput == control == js["Throughput(Control)"]
                assert js["Num_of_reads"] == sum(1 for v in want.values() if v[2]) and js["Throughput"] == sum(v[0] for v in want.values() if v[2])
                p.close()
            if n_zmw == 300:
                continue
            n_rec = len(scraps) + len(subreads)
            res = {"metric": "seconds from *.scraps.bam + *.subreads.bam to run_platformqc's JSON block and figure data", "unit": "s", "n_zmw": n_zmw, "records": n_rec,
                   "inflated_bytes": sum(len(s) for s in streams), "reps": a.reps, "value": round(statistics.median(t["file_to_json_host_inflate_all_s"]), 4),
                   "device": {k: spread(v) for k, v in t.items() if k != "python_model_s"},
                   "records_per_s_from_inflated_bytes": round(n_rec / (statistics.median(t["add_bytes_s"]) + statistics.median(t["finish_s"]))),
                   "kernel_stages_ms": kernel_stages(n_zmw), "python_model_on_this_host": spread(t["python_model_s"]), "results_equal": True, "stats": fig["stats"]}
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    if os.environ.get("OUT"):
        os.makedirs(os.environ["OUT"], exist_ok=True)
        with open(os.path.join(os.environ["OUT"], "sequel_time.json"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

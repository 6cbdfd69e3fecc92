#!/usr/bin/env python3
"""The BAM reader (csrc/reader.cpp, bgzf.hpp, kernels_bam.hpp) on random files written by tests/bam_writer.py: random reads over all
16 codes, names, cigars, tag blobs, flags, qualities (some records without), header texts and references, block sizes, stored and
deflated blocks, empty blocks, files without the EOF marker, piece sizes, thread counts, chunk sizes and both quality modes.  Every
chunk's records must be the written list cut by lq_utils.parse_bam_chunk's rule.
--inflate device: the blocks are inflated by k_bgzf_inflate (FileChunks(inflate="device")); the files then also take level 9 and the
strategies Z_FIXED, Z_RLE and Z_HUFFMAN_ONLY, and every case is read in host mode as well: the two modes must give the same chunks.
    python tools/fuzz_bam.py [--n 300] [--seed 1] [--inflate device]        (the emulator build: no GPU needed)
--host-copy needed: the reads of every case also go, as FASTQ text, into a BGZF file of the same block layout -- the text input the
mode is for -- and FileChunks(inflate="device", parse="device") must give the same chunks, or the same error, with host_copy="needed"
as with "all" and as the host modes (a BAM file itself ignores the mode while its record walk is the host's).
--walk device: the BAM's records are found on the device (FileChunks(bam_walk="device"): k_bam_*); every case must give the written
list, and with --inflate device --host-copy needed the BAM reader itself keeps the inflated bytes on the device (copy_stats: active).
The text detour of --host-copy needed is left out then: the mode is the BAM reader's own.  The last line reports how many records the device vouched for and how many the host walk took.
    python tools/fuzz_bam.py --walk device [--inflate device --host-copy needed]"""
import argparse
import os
import random
import sys
import struct
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lib", default=os.environ.get("LQCOV_EMU_LIB") or os.path.join(ROOT, "tests", "emu", "liblqcov_emu.so"))
    ap.add_argument("--inflate", choices=("host", "device"), default="host")
    ap.add_argument("--host-copy", choices=("all", "needed"), default="all")
    ap.add_argument("--walk", choices=("host", "device"), default="host")
    args = ap.parse_args()
    from longqc_amd import api, chunkpass
    from tests import bam_writer as BW
    lib = api.load_library(args.lib)
    rng = random.Random(args.seed)
    bad, on_device, on_host = 0, 0, 0
    bam_kw = dict(bam_walk="device", host_copy=args.host_copy) if args.walk == "device" else {}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "f.bam")
        for it in range(args.n):
            n = rng.choice((0, 1, 2, rng.randint(3, 80)))
            top = rng.choice((3, 40, 300, 20000))
            reads, quals, cigars, tags, flags = [], [], [], [], []
            for i in range(n):
                l = rng.choice((0, 1, rng.randint(0, top)))
                reads.append([bytes(rng.randint(33, 126) if rng.random() > 0.1 else 32 for _ in range(rng.randint(1, 60))),
                              bytes(rng.choices(BW.CODES, k=l))])
                quals.append(None if rng.random() < 0.2 else bytes(rng.choices(range(94), k=l)))
                cigars.append([rng.randrange(1 << 32) for _ in range(rng.choice((0, 0, 1, 5)))])
                tags.append(bytes(rng.choices(range(256), k=rng.choice((0, 3, 70, 2 * l)))))
                flags.append(rng.randrange(1 << 12))
            kw = dict(block_payload=rng.choice((1, 2, 3, 37, 100, 4096, 60000, 65280)), level=rng.choice((0, 1, 6)),
                      header_text=bytes(rng.choices(b"@HDSQ\tVN:1.5\n", k=rng.choice((0, 10, 5000)))),
                      refs=[(b"c%d" % i, i) for i in range(rng.choice((0, 0, 1, 200)))], eof=rng.random() < 0.7,
                      empty_block_every=rng.choice((0, 0, 1, 5)))
            if args.inflate == "device":                            # bam_writer's blocks with a strategy of zlib's
                kw["level"], kw["strategy"] = rng.choice((0, 1, 6, 9)), rng.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY))
                stream = BW.bam_stream(reads, quals, kw["header_text"], kw["refs"], cigars, tags, flags)
                with open(path, "wb") as f:
                    for k, i in enumerate(range(0, len(stream), kw["block_payload"])):
                        data = [b""] * (kw["empty_block_every"] and k % kw["empty_block_every"] == kw["empty_block_every"] - 1) + [stream[i:i + kw["block_payload"]]]
                        for part in data:
                            c = zlib.compressobj(kw["level"], zlib.DEFLATED, -15, 9, kw["strategy"])
                            body = c.compress(part) + c.flush()
                            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body
                                    + struct.pack("<II", zlib.crc32(part) & 0xffffffff, len(part)))
                    if kw["eof"]:
                        f.write(BW.EOF_BLOCK)
            else:
                BW.write_bam(path, reads, quals, cigars=cigars, tags=tags, flags=flags, **kw)
            piece, threads, ov, sequel = rng.choice((None, 16, 100, 4096)), rng.choice((0, 1, 2, 3, 16)), rng.choice((49, 41)), rng.random() < 0.5
            size = sum(3 * ov + len(r[0]) + 2 * len(r[1]) for r in reads)
            cs = rng.choice((1 << 40, 1, size // 3 + 1, max(size, 1)))
            if piece:
                os.environ["LQREADER_PIECE_BYTES"] = str(piece)
            else:
                os.environ.pop("LQREADER_PIECE_BYTES", None)
            want_r = [[r[0].decode(), r[1].decode(), "!" * len(r[1]) if sequel or q is None or not r[1] else bytes(x + 33 for x in q).decode("latin-1")]
                      for r, q in zip(reads, quals)]
            want, cur, acc, ns, nb = [], [], 0, 0, 0
            for r in want_r:
                cur.append(r); acc += 3 * ov + len(r[0]) + 2 * len(r[1]); ns += 1; nb += len(r[1])
                if acc >= cs:
                    want.append((cur, ns, nb)); cur, acc = [], 0
            want.append((cur, ns, nb))
            try:
                fc = chunkpass.FileChunks(path, chunk_size=cs, str_overhead=ov, lib=lib, n_threads=threads, is_sequel=sequel, inflate=args.inflate, **bam_kw)
                got = [(ch.records(), a, b) for ch, a, b in fc]
                ok = got == want and fc.format == 1
                if args.walk == "device":
                    ps = fc.parse_stats
                    on_device += ps["records_device"]; on_host += ps["records_host"]
                    ok = ok and ps["records_device"] + ps["records_host"] == n and ps["fallbacks"] == 0
                    ok = ok and fc.copy_stats["active"] == int(args.inflate == "device" and args.host_copy == "needed")
                if ok and args.inflate == "device":
                    ok = got == [(ch.records(), a, b) for ch, a, b in chunkpass.FileChunks(path, chunk_size=cs, str_overhead=ov, lib=lib, n_threads=threads,
                                                                                         is_sequel=sequel, inflate="host")]
            except api.LqcovError as e:
                got, ok = repr(e), False
            if ok and args.host_copy == "needed" and args.walk == "host":      # (--walk device: the BAM reader itself has just honoured the mode)
                text = b"".join(b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + (b"!" * len(r[1]) if q is None else bytes(x + 33 for x in q)) + b"\n" for r, q in zip(reads, quals))
                tpath = os.path.join(d, "f.fq.gz")
                open(tpath, "wb").write(BW.bgzf(text, block_payload=kw["block_payload"], level=min(kw["level"], 6), eof=kw["eof"], empty_block_every=kw["empty_block_every"]))
                res = []
                for mode in (dict(inflate="host", parse="host"), dict(inflate="device", parse="device", host_copy="all"), dict(inflate="device", parse="device", host_copy="needed")):
                    try:
                        fc = chunkpass.FileChunks(tpath, chunk_size=cs, str_overhead=ov, lib=lib, n_threads=threads, **mode)
                        res.append([(ch.records(), a, b) for ch, a, b in fc])
                    except api.LqcovError as e:
                        res.append(str(e))
                ok = res[0] == res[1] == res[2] and fc.copy_stats["active"] == (1 if os.path.getsize(tpath) else 0)      # (no byte: not a gzip file)
                if not ok:
                    got = "the text of the reads: host_copy=needed differs"
            if not ok:
                bad += 1
                print("case %d: %d reads, %s, piece %s, %d threads, chunk_size %d, is_sequel %s: %s" % (
                    it, n, kw if len(kw["header_text"]) < 50 else "...", piece, threads, cs, sequel,
                    got if isinstance(got, str) else [(len(c), a, b) for c, a, b in got]))
    if args.walk == "device":
        print("records the device vouched for: %d; records the host walk took: %d" % (on_device, on_host))
    print("%d cases, %d failed" % (args.n, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

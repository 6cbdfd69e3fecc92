#!/usr/bin/env python3
"""The two FASTA/FASTQ readers on random text: the streaming reader (csrc/fastx.hpp, kseq's grammar, kseq.h:179-224) and the
mapped-file reader (csrc/fastx_mem.hpp: pieces parsed by several threads from guessed record starts) must report the same
records -- count, bases, and the two digests of names+sequences and of qualities -- on every input, however malformed.
    python tools/fuzz_reader.py [--n 20000] [--seed 1]        (host code only: any build of the library will do)
--inflate device: gzip cases instead, as tools/fuzz_bam.py has them for BGZF -- record texts compressed by zlib at random level, memLevel,
strategy and flush points, as one or several members, some with a damaged byte, a cut end or bytes behind the last member; each is
read by FileChunks in host mode (gzread) and in device mode (speculative spans, csrc/gzip.hpp) at a random span length, and the
records, the counts and the error must be the same.
    python tools/fuzz_reader.py --inflate device [--n 300] [--seed 1]        (the emulator build, or the GPU's with --lib)
--parse device: the token soup and the damaged records of the default mode, each read by FileChunks with parse="host" and with
parse="device" (the record scan k_fx_*, csrc/kernels_fxscan.hpp) at a random piece length and chunk size: the chunks, names, records and
the error must be the same; and chunkpass.scan_records' rows must be a prefix of the records the host parser reads.
    python tools/fuzz_reader.py --parse device [--n 2000] [--seed 1]         (the emulator build, or the GPU's with --lib)
--parse device --host-copy needed: the same inputs as bgzip (even cases, blocks of a random size) or gzip files, read by the host
modes and by FileChunks(inflate="device", parse="device", host_copy="needed"), where the inflated bytes stay on the device
(k_crc32_ranges, k_fx_names): the same chunks, names, records and errors."""
import argparse
import gzip
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gzip_cases(lib, n, seed):
    import random
    import zlib
    from longqc_amd import api, chunkpass
    rng = random.Random(seed)

    def text():
        recs = []
        for r in range(rng.randrange(1, 400)):
            L = rng.randrange(0, 3000) if rng.random() < 0.2 else rng.randrange(0, 200)
            s = bytes(rng.choices(b"ACGTN", k=L))
            if rng.random() < 0.3:
                recs.append(b">r%d c\n" % r + s + b"\n")
            else:
                recs.append(b"@r%d\n" % r + s + b"\n+\n" + bytes(rng.choices(b"#$%&'()*+,-./0123456789:;<=>?@ABCDEFGHI", k=L)) + b"\n")
        return b"".join(recs)

    def member(data):
        c = zlib.compressobj(rng.choice((0, 1, 1, 6, 6, 6, 9)), zlib.DEFLATED, 31, rng.randrange(1, 10),
                             rng.choice((zlib.Z_DEFAULT_STRATEGY,) * 4 + (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED)))
        if rng.random() < 0.7:
            return c.compress(data) + c.flush()
        step, out = rng.randrange(500, 20000), []
        for i in range(0, len(data), step):
            out.append(c.compress(data[i:i + step]) + c.flush(rng.choice((zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH))))
        return b"".join(out) + c.flush()

    def read(path, mode):
        try:
            fc = chunkpass.FileChunks(path, chunk_size=rng_cs, lib=lib, str_overhead=49, inflate=mode)
            return [(ch.records(), ns, nb) for ch, ns, nb in fc], None
        except api.LqcovError as e:
            return None, (e.code, str(e))

    bad = 0
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "f.fq.gz")
        for it in range(n):
            data = bytearray(b"".join(member(text()) for _ in range(rng.choice((1, 1, 1, 2, 3)))))
            kind = rng.randrange(6)
            if kind == 1:
                data[rng.randrange(len(data))] ^= 1 << rng.randrange(8)
            elif kind == 2:
                del data[rng.randrange(len(data)):]
            elif kind == 3:
                data += rng.choice((bytes(rng.randrange(1, 200)), b"@x\nACGT\n+\nIIII\n", b"\x1f", b"\x1f\x8b", b"\x1f\x8b\x08\x00"))
            open(fn, "wb").write(bytes(data))
            os.environ["LQREADER_GZ_SPAN_BYTES"] = str(rng.choice((1024, 2048, 4096, 16384)))
            rng_cs = rng.choice((1 << 40, 20000, 100000))
            host, dev = read(fn, "host"), read(fn, "device")
            # (an error: the code and the message; how many chunks came before it is not compared)
            if host != dev:
                bad += 1
                print("case %d (kind %d, %d bytes, span %s) differs: host %s, device %s" % (it, kind, len(data), os.environ["LQREADER_GZ_SPAN_BYTES"],
                      host[1] or len(host[0]), dev[1] or len(dev[0])))
                open("fuzz_reader_case_%d.gz" % it, "wb").write(bytes(data))
                if bad >= 5:
                    break
    print("%d gzip inputs, %d on which host and device mode disagree" % (it + 1, bad))
    return 1 if bad else 0


def soup(rng, toks):
    kind = rng.integers(0, 3)
    if kind == 0:                           # token soup
        return b"".join(toks[i] for i in rng.integers(0, len(toks), size=int(rng.integers(0, 60))))
    recs = []                               # mostly well-formed records with a few damaged bytes
    for r in range(int(rng.integers(1, 8))):
        L = int(rng.integers(0, 40))
        s = bytes(rng.choice(list(b"ACGTN"), size=L).astype(np.uint8)) if L else b""
        eol = b"\r\n" if rng.random() < 0.2 else b"\n"
        w = int(rng.integers(1, 30))
        wrapped = rng.random() < 0.5 and L
        if rng.random() < 0.5:
            recs.append(b">r%d c" % r + eol + (eol.join(s[i:i + w] for i in range(0, len(s), w)) if wrapped else s) + eol)
        else:
            q = bytes(rng.integers(33, 74, size=L).astype(np.uint8)) if L else b""   # (qualities may hold '@', '>' and '+')
            if wrapped:
                s, q = eol.join(s[i:i + w] for i in range(0, L, w)), eol.join(q[i:i + w + 1] for i in range(0, L, w + 1))
            recs.append(b"@r%d" % r + eol + s + eol + b"+" + eol + q + eol)
    data = bytearray(b"".join(recs))
    for _ in range(int(rng.integers(0, 3)) if kind == 2 else 0):
        if data:
            data[int(rng.integers(0, len(data)))] = int(rng.choice(list(b">@+\n\r A!")))
    if rng.random() < 0.2 and data:
        data = data[:int(rng.integers(0, len(data)))]      # truncated
    return bytes(data)


def parse_cases(lib, n, seed, host_copy="all"):
    from longqc_amd import api, chunkpass
    from tests import bam_writer
    needed = host_copy == "needed"
    kw_dev = dict(parse="device", inflate="device", host_copy="needed") if needed else dict(parse="device")
    kw_host = dict(parse="host", inflate="host") if needed else dict(parse="host")
    rng = np.random.default_rng(seed)
    toks = [b">", b"@", b"+", b"\n", b"\n", b"\n", b"\r\n", b"\r", b"\r\r\n", b" ", b"\t", b"ACGT", b"acgtnN", b"U", b"!!!!", b"IIII", b"@@", b">>", b"+\n", b"name", b"x y", b""]

    active = 0

    def read(path, kw, cs):
        nonlocal active
        try:
            fc = chunkpass.FileChunks(path, chunk_size=cs, lib=lib, str_overhead=49, **kw)
            out = [(ch.records(), list(ch.names), ns, nb) for ch, ns, nb in fc]
            active += fc.copy_stats["active"]
            return out, None
        except api.LqcovError as e:
            return None, (e.code, str(e))

    bad, vouched, total = 0, 0, 0
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "f.txt")
        for it in range(n):
            data = soup(rng, toks)
            if not needed:
                open(fn, "wb").write(data)
            elif it % 2 == 0:
                open(fn, "wb").write(bam_writer.bgzf(data, block_payload=int(rng.choice((1, 7, 37, 100, 65280))), level=int(rng.choice((0, 1, 6)))))
            else:
                open(fn, "wb").write(gzip.compress(data, int(rng.choice((1, 6)))))
            os.environ["LQREADER_PIECE_BYTES"] = str(rng.choice((16, 40, 100, 1 << 20)))
            cs = int(rng.choice((1 << 40, 1, 300)))
            host, dev = read(fn, kw_host, cs), read(fn, kw_dev, cs)
            ok = host == dev
            if ok and host[0] is not None:
                names = [x for c in host[0] for x in c[1]]
                rows = chunkpass.scan_records(data, lib=lib)[0]
                ok = [data[a:a + l].decode("ascii", "replace") for a, l, _, _ in rows.tolist()] == names[:rows.shape[0]]
                vouched += rows.shape[0]; total += len(names)
            if not ok:
                bad += 1
                print("case %d differs (piece %s, chunk size %d): %r\n  host %s\n  device %s" % (it, os.environ["LQREADER_PIECE_BYTES"], cs, data, host, dev))
                if bad >= 5:
                    break
    print("%d inputs, %d on which the host and the device parse disagree; the device vouched for %d of %d records" % (it + 1, bad, vouched, total))
    if needed:
        print("host_copy=needed was active for %d of them" % active)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lib", default=os.environ.get("LQCOV_EMU_LIB") or os.path.join(ROOT, "tests", "emu", "liblqcov_emu.so"))
    ap.add_argument("--inflate", choices=("host", "device"), default="host")
    ap.add_argument("--parse", choices=("host", "device"), default="host")
    ap.add_argument("--host-copy", choices=("all", "needed"), default="all", help="with --parse device: bgzip and gzip inputs, the inflated bytes stay on the device")
    args = ap.parse_args()
    from longqc_amd import api
    lib = api.load_library(args.lib)
    if args.parse == "device":
        sys.exit(parse_cases(lib, args.n if args.n != 20000 else 2000, args.seed, args.host_copy))
    if args.inflate == "device":
        sys.exit(gzip_cases(lib, args.n if args.n != 20000 else 300, args.seed))
    rng = np.random.default_rng(args.seed)
    toks = [b">", b"@", b"+", b"\n", b"\n", b"\n", b"\r\n", b"\r", b" ", b"\t", b"ACGT", b"acgtnN", b"U", b"!!!!", b"IIII", b"@@", b">>", b"+\n", b"name", b"x y", b""]
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "f.txt")
        for it in range(args.n):
            kind = rng.integers(0, 3)
            if kind == 0:                           # token soup
                data = b"".join(toks[i] for i in rng.integers(0, len(toks), size=int(rng.integers(0, 60))))
            else:                                   # mostly well-formed records with a few damaged bytes
                recs = []
                for r in range(int(rng.integers(1, 8))):
                    L = int(rng.integers(0, 40))
                    s = bytes(rng.choice(list(b"ACGTN"), size=L).astype(np.uint8)) if L else b""
                    eol = b"\r\n" if rng.random() < 0.2 else b"\n"
                    if rng.random() < 0.5:
                        w = int(rng.integers(1, 30))
                        body = eol.join(s[i:i + w] for i in range(0, len(s), w)) if rng.random() < 0.5 and L else s
                        recs.append(b">r%d c" % r + eol + body + eol)
                    else:
                        q = bytes(rng.integers(33, 74, size=L).astype(np.uint8)) if L else b""   # (qualities may hold '@', '>' and '+')
                        recs.append(b"@r%d" % r + eol + s + eol + b"+" + eol + q + eol)
                data = bytearray(b"".join(recs))
                for _ in range(int(rng.integers(0, 3)) if kind == 2 else 0):
                    if data:
                        data[int(rng.integers(0, len(data)))] = int(rng.choice(list(b">@+\n\r A!")))
                if rng.random() < 0.2 and data:
                    data = data[:int(rng.integers(0, len(data)))]      # truncated
                data = bytes(data)
            open(fn, "wb").write(data)
            got = []
            for mode, th, piece in ((0, 1, 0), (1, 4, 16), (1, 3, 7)):
                out = (C.c_uint64 * 5)()
                rc = lib.lqcov_fastx_digest(fn.encode(), mode, th, piece, out)
                got.append((rc,) + tuple(int(x) for x in out)[:4])        # (out[4]: pieces parsed again, the parallel reader's own business)
            if len(set(got)) != 1:
                bad += 1
                print("case %d differs: %r\n  streaming %s\n  mapped/4/16 %s\n  mapped/3/7 %s" % (it, data, got[0], got[1], got[2]))
                if bad >= 5:
                    break
    print("%d inputs, %d on which the readers disagree" % (it + 1, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

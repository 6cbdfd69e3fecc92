#!/usr/bin/env python3
"""The BAM reader (csrc/reader.cpp, bgzf.hpp, kernels_bam.hpp) on random files written by tests/bam_writer.py: random reads over all
16 codes, names, cigars, tag blobs, flags, qualities (some records without), header texts and references, block sizes, stored and
deflated blocks, empty blocks, files without the EOF marker, piece sizes, thread counts, chunk sizes and both quality modes.  Every
chunk's records must be the written list cut by lq_utils.parse_bam_chunk's rule.
    python tools/fuzz_bam.py [--n 300] [--seed 1]        (the emulator build: no GPU needed)"""
import argparse
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lib", default=os.environ.get("LQCOV_EMU_LIB") or os.path.join(ROOT, "tests", "emu", "liblqcov_emu.so"))
    args = ap.parse_args()
    from longqc_amd import api, chunkpass
    from tests import bam_writer as BW
    lib = api.load_library(args.lib)
    rng = random.Random(args.seed)
    bad = 0
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
                fc = chunkpass.FileChunks(path, chunk_size=cs, str_overhead=ov, lib=lib, n_threads=threads, is_sequel=sequel)
                got = [(ch.records(), a, b) for ch, a, b in fc]
                ok = got == want and fc.format == 1
            except api.LqcovError as e:
                got, ok = repr(e), False
            if not ok:
                bad += 1
                print("case %d: %d reads, %s, piece %s, %d threads, chunk_size %d, is_sequel %s: %s" % (
                    it, n, kw if len(kw["header_text"]) < 50 else "...", piece, threads, cs, sequel,
                    got if isinstance(got, str) else [(len(c), a, b) for c, a, b in got]))
    print("%d cases, %d failed" % (args.n, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

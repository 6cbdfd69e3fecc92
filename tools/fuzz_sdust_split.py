#!/usr/bin/env python3
"""The scan in pieces (lqchunk_sdust_split, kernels_dust_split.hpp) against the reference binary: random sets of reads -- random bases,
homopolymers, short tandem repeats, two-letter stretches, lower case, repeats of longer units; some sets free of any byte but A/C/G/T,
some with N runs and other letters -- random `-w` / `-t` and a random piece from 2 W + 2 bases up, through the emulator build (tests/emu)
and through oracle/_ref/sdust; the masked-bases column must be the same for every read, whichever walk it took, and the intervals of the
reads the pieces serve must add up to it.  The emulator's thread order is drawn per set as well (LQ_EMU_ORDER).
    python tools/fuzz_sdust_split.py [--n 300] [--seed 1]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lib", default=os.environ.get("LQCOV_EMU_LIB") or os.path.join(ROOT, "tests", "emu", "liblqcov_emu.so"))
    args = ap.parse_args()
    from longqc_amd import api, chunkpass
    from tests import oracle_bind
    lib = api.load_library(args.lib)
    ref = os.path.join(os.path.dirname(oracle_bind.REF_BIN), "sdust")
    rng = np.random.default_rng(args.seed)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    bad = n_cut = n_serial = 0
    with tempfile.TemporaryDirectory() as d:
        for it in range(args.n):
            W = int(rng.choice([3, 8, 16, 20, 32, 50, 64, 66]))
            T = int(rng.choice([5, 12, 20, 30, 40]))
            piece = 2 * W + 2 + int(rng.integers(0, 3)) * int(rng.integers(0, 120))
            with_other = rng.random() < 0.4                          # the set holds reads with N and other letters
            reads = []
            for r in range(int(rng.integers(1, 10))):
                parts = []
                for _ in range(int(rng.integers(1, 10))):
                    kind = int(rng.integers(0, 7))
                    L = int(rng.integers(1, 500))
                    if kind == 0:
                        parts.append(A[rng.integers(0, 4, L)])
                    elif kind == 1:
                        parts.append(np.full(L, A[rng.integers(0, 4)], dtype=np.uint8))
                    elif kind == 2:
                        u = A[rng.integers(0, 4, int(rng.integers(2, 7)))]
                        parts.append(np.tile(u, L // len(u) + 1)[:L])
                    elif kind == 3:
                        parts.append(A[rng.integers(0, 4, 2)][rng.integers(0, 2, L)])
                    elif kind == 4:
                        parts.append(np.frombuffer(bytes(A[rng.integers(0, 3, L)]).lower(), dtype=np.uint8))
                    elif kind == 5:
                        u = A[rng.integers(0, 4, int(rng.integers(8, 40)))]
                        parts.append(np.tile(u, int(rng.integers(2, 6))))
                    elif with_other and rng.random() < 0.5:
                        parts.append(np.frombuffer(b"NnURY", dtype=np.uint8)[rng.integers(0, 5, int(rng.integers(1, 4)))])
                s = np.concatenate(parts) if parts else A[rng.integers(0, 4, 5)]
                if rng.random() < 0.05:
                    s = s[:int(rng.integers(1, 5))]
                reads.append(s)
            fn = os.path.join(d, "r.fa")
            with open(fn, "wb") as f:
                for i, s in enumerate(reads):
                    f.write(b">s%d\n" % i + s.tobytes() + b"\n")
            a = subprocess.run([ref, "-w", str(W), "-t", str(T), fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            want = [int(l.split(b"\t")[1]) for l in a.stdout.splitlines()]
            order = ["", "reverse", "random:%d" % it][int(rng.integers(0, 3))]
            os.environ.pop("LQ_EMU_ORDER", None)
            if order:
                os.environ["LQ_EMU_ORDER"] = order
            ch = chunkpass.ReadChunk([["s%d" % i, s.tobytes().decode()] for i, s in enumerate(reads)], lib=lib)
            got = ch.sdust(W, T, split="pieces", piece=piece)[0][:len(reads)].tolist()
            n_serial += ch.n_serial
            n_cut += len(reads) - ch.n_serial
            iv_off, iv, flagged = ch.sdust_intervals(W, T, piece)
            sums = [int((iv[int(iv_off[i]):int(iv_off[i + 1]), 1] - iv[int(iv_off[i]):int(iv_off[i + 1]), 0]).sum()) for i in range(len(reads))]
            ch.close()
            ok = got == want and all(f or s == w for f, s, w in zip(flagged, sums, want))
            if not ok:
                bad += 1
                print("set %d differs (-w %d -t %d, piece %d, order %r): lengths %s\n  reference %s\n  pieces    %s\n  intervals %s flagged %s"
                      % (it, W, T, piece, order, [len(s) for s in reads], want, got, sums, flagged.astype(int).tolist()))
                if bad >= 5:
                    break
    print("%d sets, %d differ; %d reads cut into pieces, %d on the serial walk" % (it + 1, bad, n_cut, n_serial))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

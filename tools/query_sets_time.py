#!/usr/bin/env python3
"""LongQC's `sampleqc --short` as two coverage calls against one call with two query sets (lqcov_run_files_sets), in one process
on one device.  configs[2]-shaped files from longqc_amd/synth.py on tmpfs: the targets (500k PacBio Sequel CLR reads ~10 kb,
FASTA), a main set of LongQC's seed-7 subsample of 4 000 reads mapped with -p 80 and a short set of 1 000 pieces of 200-499
bases cut from target reads, mapped with -p 60 (pb-sequel's pair, sampleqc.PRESET_MED_SCORE), -q 160 for both.  Each call
gets a handle of its own, as each call of the executable is a process of its own; a small call first takes the device's
start-up out of the figures.  The walls are the best of --reps alternating rounds.  Checks that both ways print the same
tables and prints one JSON line.
Usage: python tools/query_sets_time.py [--reps 2] [--dir /dev/shm] [--workers 16] [--gz]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from longqc_amd import api, synth  # noqa: E402

ARGV = ["-Y", "-l", "0", "-q", "160", "-k", "12", "-w", "5", "-I", "4G", "-t", "4"]
MED = (80, 60)


def make_files(d, workers, n_main=4000, n_short=1000, seed=11):
    """-> (main.fq, short.fq, all.fa): configs[2]'s reads, the subsample and the short pieces (qualities '!', as Sequel CLR's)"""
    cfg = synth.CONFIGS["cfg3"]
    F = synth.make_reads_flat(cfg, synth.make_genome(cfg), workers=workers)
    paths = [os.path.join(d, "main.fq"), os.path.join(d, "short.fq"), os.path.join(d, "all.fa")]
    synth.write_flat_fasta(paths[2], F)
    names = F.names()
    with open(paths[0], "wb") as f:
        for i in synth.reservoir_subsample(len(F), n_main):
            s = F.seq(i).tobytes()
            f.write(b"@%s\n%s\n+\n%s\n" % (names[i].encode(), s, b"!" * len(s)))
    rng = np.random.default_rng(seed)
    with open(paths[1], "wb") as f:
        for j, i in enumerate(rng.choice(len(F), size=n_short, replace=False)):
            s = F.seq(int(i))
            L = int(rng.integers(200, 500))
            a = int(rng.integers(0, max(1, s.shape[0] - L)))
            piece = s[a:a + L].tobytes()
            f.write(b"@short%d_%s\n%s\n+\n%s\n" % (j, names[int(i)].encode(), piece, b"!" * len(piece)))
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--gz", action="store_true", help="also time a gzip-compressed target (one round)")
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix="lqsets_", dir=args.dir)
    try:
        t0 = time.time()
        main_fq, short_fq, target = make_files(d, args.workers)
        t_data = time.time() - t0

        def engine(med):
            p, _, _ = api.parse_args(ARGV + ["-p", str(med), "t", "q"])
            return api.Engine(p, device=0)

        def two_calls(tgt):
            t = time.time()
            texts = []
            for fq, med in zip((main_fq, short_fq), MED):
                eng = engine(med)
                o = os.path.join(d, "sep_%d.tsv" % med)
                eng.run_files(tgt, fq, out=o, err=os.path.join(d, "sep.err"))
                eng.close()
                texts.append(open(o).read())
            return time.time() - t, texts

        def one_call(tgt):
            t = time.time()
            eng = engine(MED[0])
            outs = [os.path.join(d, "set_%d.tsv" % k) for k in range(2)]
            eng.run_files_sets(tgt, [main_fq, short_fq], list(MED), [160, 160], outs, err=os.path.join(d, "sets.err"))
            eng.close()
            return time.time() - t, [open(o).read() for o in outs]

        warm = engine(MED[0])                                  # device start-up, kernels loaded
        warm.run_files(short_fq, short_fq, out=os.path.join(d, "warm.tsv"), err=os.path.join(d, "warm.err"))
        warm.close()
        walls_two, walls_one, same = [], [], True
        for _ in range(max(1, args.reps)):
            w2, sep = two_calls(target)
            w1, sets = one_call(target)
            walls_two.append(w2); walls_one.append(w1)
            same = same and sep == sets
        res = dict(tool="query_sets_time", config="cfg3", n_main=4000, n_short=1000, med=list(MED), good=160,
                   data_s=round(t_data, 1), two_calls_s=[round(x, 3) for x in walls_two], one_call_s=[round(x, 3) for x in walls_one],
                   two_calls_best_s=round(min(walls_two), 3), one_call_best_s=round(min(walls_one), 3),
                   ratio=round(min(walls_one) / min(walls_two), 3), tables_identical=bool(same),
                   rows=[len(t.splitlines()) for t in sets])
        if args.gz:
            import gzip
            gz = target + ".gz"
            with open(target, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
                shutil.copyfileobj(f, g)
            w2, sep = two_calls(gz)
            w1, sets = one_call(gz)
            res.update(gz_two_calls_s=round(w2, 3), gz_one_call_s=round(w1, 3), gz_tables_identical=sep == sets)
            same = same and sep == sets
        print(json.dumps(res))
        return 0 if same else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

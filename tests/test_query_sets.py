"""Several query sets in one pass over the targets, each set with its own -p / -q (lqcov_set_query_sets,
lqcov_run_files_sets): LongQC's `sampleqc --short` maps the same targets with the same index options twice, once per
subsample, and only the query file and -p differ (longQC.py:438-445,527-543; the spike-in filter, :553-575).  Every set's
table must be byte for byte the table of a call of its own."""
import gzip
import os
import shutil

import numpy as np
import pytest

from longqc_amd import api
from tests import oracle_bind
from tests.conftest import GOLDEN, read_gz
from tests.helpers import read_fastx, run_main

TINY = ["-Y", "-l", "0", "-q", "160", "-k", "12", "-w", "5", "-I", "4G", "-t", "4"]          # tiny_ont / tiny_pb without -p
ADV_PARTS = ["-Y", "-l", "0", "-q", "160", "-k", "12", "-w", "5", "-I", "100K", "-t", "4"]    # adv_parts without -p
SPIKE = ["-Y", "-Hk15", "-w", "10", "-c", "1", "-l", "0", "--filter", "-t", "4"]                # tiny_spike


def _engine(lib, argv):
    p, _, _ = api.parse_args(argv + ["t", "q"])
    return api.Engine(p, device=0, lib=lib)


def _gunzip(name, tmp_path):
    out = str(tmp_path / name[:-3])
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f, open(out, "wb") as o:
        shutil.copyfileobj(f, o)
    return out


def _write_fastq(path, names, seqs, quals):
    with open(path, "wb") as f:
        for n, s, q in zip(names, seqs, quals):
            f.write(b"@" + n.encode() + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return path


def _split_by_median(tmp_path):
    """adv_sub.fq.gz cut at its median length: the reads of at least that length and the shorter ones, as two FASTQ files"""
    names, seqs, quals = read_fastx(os.path.join(GOLDEN, "adv_sub.fq.gz"))
    med = int(np.median([len(s) for s in seqs]))
    lo = [i for i in range(len(seqs)) if len(seqs[i]) < med]
    hi = [i for i in range(len(seqs)) if len(seqs[i]) >= med]
    assert lo and hi
    pick = lambda ix: ([names[i] for i in ix], [seqs[i] for i in ix], [quals[i] for i in ix])
    return (_write_fastq(str(tmp_path / "long.fq"), *pick(hi)), _write_fastq(str(tmp_path / "short.fq"), *pick(lo)))


def check_tiny_two_thresholds(lib, tmp_path):
    """the same subsample twice, -p 160 and -p 80: the two golden tables (they differ in column 5), and write_table their concatenation"""
    outs = [str(tmp_path / "s0.tsv"), str(tmp_path / "s1.tsv")]
    eng = _engine(lib, TINY + ["-p", "160"])
    q = os.path.join(GOLDEN, "tiny_sub.fq.gz")
    eng.run_files_sets(os.path.join(GOLDEN, "tiny_all.fq.gz"), [q, q], [160, 80], [160, 160], outs, err=str(tmp_path / "err"))
    ont, pb = read_gz("tiny_ont.table.gz"), read_gz("tiny_pb.table.gz")
    assert ont != pb
    assert open(outs[0]).read() == ont
    assert open(outs[1]).read() == pb
    assert eng.n_query_sets == 2
    assert eng.table_text(set=0) == ont and eng.table_text(set=1) == pb
    assert eng.table_text() == ont + pb
    err = open(str(tmp_path / "err")).read()
    assert "min-score-med 160" in err and "query set 1:" in err and "min-score-med 80, min-score-good 160" in err
    eng.close()


def check_adv_parts_split(lib, tmp_path):
    """adv_parts' argv (several index parts, COVT across them) with the subsample split at its median length, -p 160 / -p 140"""
    long_fq, short_fq = _split_by_median(tmp_path)
    target = os.path.join(GOLDEN, "adv_all.fa.gz")
    outs = [str(tmp_path / "long.tsv"), str(tmp_path / "short.tsv")]
    eng = _engine(lib, ADV_PARTS + ["-p", "160"])
    eng.run_files_sets(target, [long_fq, short_fq], [160, 140], [160, 160], outs)
    eng.close()
    want = [oracle_bind.table(ADV_PARTS + ["-p", "160", target, long_fq]), oracle_bind.table(ADV_PARTS + ["-p", "140", target, short_fq])]
    assert want[0] and want[1]
    assert open(outs[0]).read() == want[0]
    assert open(outs[1]).read() == want[1]


def test_tiny_sets_with_two_thresholds_equal_the_golden_tables(emu_lib, tmp_path):
    check_tiny_two_thresholds(emu_lib, tmp_path)


def test_adv_parts_long_and_short_sets(emu_lib, tmp_path):
    check_adv_parts_split(emu_lib, tmp_path)


def test_in_memory_sets_over_parts_equal_separate_calls(emu_lib):
    """lqcov_set_query_sets + the part calls: the spike-in argv (--filter, -H, k 15), the subsample twice, the second time in
    reverse order; each set's table equals a run of its own, and the per-set table keeps the set's own order"""
    tn, ts, _ = read_fastx(os.path.join(GOLDEN, "tiny_all.fq.gz"))
    qn, qs, qq = read_fastx(os.path.join(GOLDEN, "tiny_sub.fq.gz"))
    rn, rs, rq = qn[::-1], qs[::-1], qq[::-1]
    eng = _engine(emu_lib, SPIKE)
    eng.set_query_sets([(qn, qs, qq, 40, 40), (rn, rs, rq, 40, 40)])
    pt = eng.part_begin()
    eng.part_add_targets(pt, tn, ts)
    eng.part_build(pt); eng.part_map(pt); eng.finish()
    got = [eng.table_text(set=0), eng.table_text(set=1)]
    eng.close()
    want = read_gz("tiny_spike.table.gz")
    assert got[0] == want
    assert got[1] == "".join(want.splitlines(True)[::-1])


def test_refusals_and_empty_set(emu_lib, tmp_path):
    qn, qs, qq = read_fastx(os.path.join(GOLDEN, "tiny_sub.fq.gz"))
    half = len(qn) // 2
    a, b = (qn[:half], qs[:half], qq[:half]), (qn[half:], qs[half:], qq[half:])

    def refused(sets, code):
        eng = _engine(emu_lib, TINY + ["-p", "160"])
        with pytest.raises(api.LqcovError) as ei:
            eng.set_query_sets(sets)
        eng.close()
        assert ei.value.code == code, str(ei.value)
        return str(ei.value)

    assert "-p must be" in refused([a + (160, 160), b + (39, 160)], -1)             # p < m (-m 40)
    assert "-q must be" in refused([a + (160, 160), b + (160, 80)], -1)             # q < p
    assert "65536" in refused([a + (160, 160), b + (160, 65536)], -1)
    assert "quer" in refused([a + (160, 160), (b[0], b[1], None, 80, 160)], -5)      # FASTQ set with a FASTA set
    eng = _engine(emu_lib, TINY + ["-p", "160"])                                     # set_first that does not cover n
    flat, off = api._flat(qs)
    nb, noff = api._names(qn)
    first = np.array([0, half, len(qs) - 1], dtype=np.uint32)
    thr = np.array([160, 80], dtype=np.int32)
    rc = emu_lib.lqcov_set_query_sets(eng.h, len(qs), flat.ctypes.data, off.ctypes.data, None, nb, noff.ctypes.data, 2,
                                      first.ctypes.data, thr.ctypes.data, np.array([160, 160], dtype=np.int32).ctypes.data)
    assert rc == -1 and "set_first" in emu_lib.lqcov_last_error(eng.h).decode()
    eng.close()
    # FASTA file with a FASTQ file through the file-level call
    fa = str(tmp_path / "q.fa")
    with open(fa, "w") as f:
        for n, s in zip(qn[:3], qs[:3]):
            f.write(">%s\n%s\n" % (n, s.tobytes().decode()))
    eng = _engine(emu_lib, TINY + ["-p", "160"])
    with pytest.raises(api.LqcovError) as ei:
        eng.run_files_sets(os.path.join(GOLDEN, "tiny_all.fq.gz"), [os.path.join(GOLDEN, "tiny_sub.fq.gz"), fa], [160, 80], [160, 160],
                           [str(tmp_path / "o0"), str(tmp_path / "o1")], err=str(tmp_path / "e"))
    assert ei.value.code == -5
    eng.close()
    # an empty set between two others: an empty table, the others as alone
    eng = _engine(emu_lib, TINY + ["-p", "160"])
    tn, ts, _ = read_fastx(os.path.join(GOLDEN, "tiny_all.fq.gz"))
    eng.set_query_sets([(qn, qs, qq, 160, 160), ([], [], None, 80, 160), (qn, qs, qq, 80, 160)])
    pt = eng.part_begin()
    eng.part_add_targets(pt, tn, ts)
    eng.part_build(pt); eng.part_map(pt); eng.finish()
    assert eng.n_query_sets == 3
    assert eng.table_text(set=1) == ""
    assert eng.table_text(set=0) == read_gz("tiny_ont.table.gz") and eng.table_text(set=2) == read_gz("tiny_pb.table.gz")
    eng.close()


# ---- several ranks (gloo on the test emulator; tests/test_multigpu_cpu.py's workers with two sets) ----
def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _adv_sets():
    """adv_sub.fq.gz split at its median length: (long set at -p 160, short set at -p 140), -q 160"""
    names, seqs, quals = read_fastx(os.path.join(GOLDEN, "adv_sub.fq.gz"))
    med = int(np.median([len(s) for s in seqs]))
    hi = [i for i in range(len(seqs)) if len(seqs[i]) >= med]
    lo = [i for i in range(len(seqs)) if len(seqs[i]) < med]
    pick = lambda ix, p: ([names[i] for i in ix], [seqs[i] for i in ix], [quals[i] for i in ix], p, 160)
    return [pick(hi, 160), pick(lo, 140)]


def _worker_sets(rank, world, port, mode, out_prefix, use_gpu=False):
    import torch
    import torch.distributed as dist
    from longqc_amd import multigpu
    from tests.conftest import ROOT
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lib = api.load_library() if use_gpu else api.load_library(os.path.join(ROOT, "tests", "emu", "liblqcov_emu.so"))
        dev = torch.device("cuda", 0) if use_gpu else torch.device("cpu")
        tn, ts, _ = read_fastx(os.path.join(GOLDEN, "adv_all.fa.gz"))
        sets = _adv_sets()
        eng = _engine(lib, ADV_PARTS + ["-p", "160"])
        lens = [int(s.shape[0]) for s in ts]
        outs = [out_prefix + ".%d" % k for k in range(len(sets))]
        if mode == "parts":                                      # index parts over ranks, the accumulators exchanged per query
            eng.set_query_sets(sets)
            runner = multigpu.PartRunner(eng, world, rank, dev, [int(s.shape[0]) for st in sets for s in st[1]])
            parts = multigpu.split_parts(lens, 100000)
            for base in range(0, len(parts), world):
                mine = base + rank
                pid = None
                if mine < len(parts):
                    s, e = parts[mine]
                    pid = eng.part_begin()
                    eng.part_add_targets(pid, tn[s:e], ts[s:e])
                    eng.part_build(pid)
                runner.map_and_combine(pid, part_index=mine, mid_occ_owner=0, share_mid_occ=(base == 0))
                if pid is not None:
                    eng.part_release(pid)
            runner.write_tables(outs)
        else:                                                    # queries over ranks, the index replicated
            runner = multigpu.QueryShardRunner(eng, world, rank, dev)
            runner.set_query_sets(sets)
            pid = eng.part_begin()
            for (s, e) in multigpu.split_parts(lens, 100000):
                lo, hi = multigpu.balanced_ranges(lens[s:e], world)[rank]
                eng.part_clear(pid)
                if hi > lo:
                    eng.part_add_targets(pid, tn[s + lo:s + hi], ts[s + lo:s + hi])
                runner.map_part(pid, lo, tn[s:e], lens[s:e])
            for k in range(len(sets)):
                t = runner.gather_table(set=k)
                if rank == 0:
                    open(outs[k], "w").write(t)
            t = runner.gather_table()
            if rank == 0:
                open(out_prefix + ".all", "w").write(t)
        eng.close()
    finally:
        dist.destroy_process_group()


def _adv_set_oracle_tables(tmp_path):
    long_fq, short_fq = _split_by_median(tmp_path)
    target = os.path.join(GOLDEN, "adv_all.fa.gz")
    return [oracle_bind.table(ADV_PARTS + ["-p", "160", target, long_fq]), oracle_bind.table(ADV_PARTS + ["-p", "140", target, short_fq])]


def check_ranks_with_sets(tmp_path, mode, use_gpu=False):
    import torch.multiprocessing as mp
    want = _adv_set_oracle_tables(tmp_path)
    out = str(tmp_path / ("t_" + mode))
    mp.spawn(_worker_sets, args=(2, _free_port(), mode, out, use_gpu), nprocs=2, join=True)
    assert open(out + ".0").read() == want[0]
    assert open(out + ".1").read() == want[1]
    if mode == "qshard":
        assert open(out + ".all").read() == want[0] + want[1]


@pytest.mark.parametrize("mode", ["parts", "qshard"])
def test_two_ranks_gloo_two_sets(emu_lib, tmp_path, mode):
    check_ranks_with_sets(tmp_path, mode)


def test_qshard_set_may_be_empty_on_a_rank():
    """the union is sharded as one set: a set of a single query has no query on one of the two ranks, which gets an empty
    set with that set's thresholds; each rank's share keeps every set's order"""
    import torch
    from longqc_amd import multigpu

    class Sink:
        def set_query_sets(self, sets):
            self.sets = sets

    seq = lambda n: np.full(n, ord("A"), np.uint8)
    sets = [(["a", "b", "c", "d"], [seq(3000), seq(2000), seq(1000), seq(900)], None, 160, 160), (["e"], [seq(800)], None, 140, 160)]
    got = []
    for rank in range(2):
        eng = Sink()
        multigpu.QueryShardRunner(eng, 2, rank, torch.device("cpu")).set_query_sets(sets)
        got.append([(list(nm), m, g) for nm, sq, ql, m, g in eng.sets])
    assert sorted(got) == [[(["a", "d"], 160, 160), ([], 140, 160)], [(["b", "c"], 160, 160), (["e"], 140, 160)]]


# ---- sampleqc: LongQC's --short split in one pass ----
def _chunks(path, chunk_reads):
    n, s, q = read_fastx(path)
    reads = [[a, b.tobytes().decode(), (c.tobytes().decode() if c is not None else "")] for a, b, c in zip(n, s, q or [None] * len(n))]
    for i in range(0, len(reads), chunk_reads):
        c = reads[i:i + chunk_reads]
        yield c, len(c), sum(len(r[1]) for r in c)


def test_sampleqc_short_split_in_one_target_pass(emu_lib, monkeypatch):
    """coverage_in_memory(short_threshold=500): adv_sub's 4 reads under 500 bases go to the short set (-p 140), the rest to the
    main one (-p 160), -I 100K (10 parts): the two tables of two separate calls, and every part is built once"""
    from longqc_amd import sampleqc
    qn, qs, qq = read_fastx(os.path.join(GOLDEN, "adv_sub.fq.gz"))
    s_reads = [[a, b.tobytes().decode(), c.tobytes().decode()] for a, b, c in zip(qn, qs, qq)]
    main_reads, short_reads = sampleqc.short_split(s_reads, 500)
    assert len(short_reads) == 4 and len(main_reads) == 16
    assert all(len(r[1]) < 500 for r in short_reads) and all(len(r[1]) >= 500 for r in main_reads)
    target = os.path.join(GOLDEN, "adv_all.fa.gz")

    def engine(short=False):
        p, _, _ = api.parse_args(sampleqc.coverage_argv("ont-ligation", "x", "y", inds="100K", short=short))
        return api.Engine(p, 0, lib=emu_lib)

    sep = []
    for reads, short in ((main_reads, False), (short_reads, True)):
        eng = engine(short)
        sep.append(sampleqc.coverage_in_memory(_chunks(target, 37), reads, inds=100000, engine=eng, short=short))
        eng.close()
    builds = []
    orig = api.Engine.part_build
    monkeypatch.setattr(api.Engine, "part_build", lambda self, part: (builds.append(part), orig(self, part))[1])
    eng = engine()
    got = sampleqc.coverage_in_memory(_chunks(target, 37), s_reads, inds=100000, engine=eng, short_threshold=500)
    eng.close()
    assert got == (sep[0], sep[1])
    assert len(builds) == 10                                      # the 10 parts of -I 100K, once each
    with pytest.raises(ValueError):
        sampleqc.coverage_in_memory([], s_reads, preset="pb-hifi", short_threshold=500)


# ---- the real library (-m gpu) ----
@pytest.mark.gpu
def test_gpu_tiny_sets_with_two_thresholds(gpu_lib, tmp_path):
    check_tiny_two_thresholds(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_adv_parts_long_and_short_sets(gpu_lib, tmp_path):
    check_adv_parts_split(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_query_sets_at_configs1_size(gpu_lib, tmp_path):
    """configs[1]-shaped targets (50k ONT reads ~15 kb), 4 000 subsampled queries at -p 160 and 1 000 reads cut to 200-499 bases
    at -p 140: each set's table equals a lqcov_run_files call of its own on the same library"""
    from longqc_amd import synth
    main_fq, short_fq, target = synth_query_sets(str(tmp_path), n_main=4000, n_short=1000)
    argv = ["-Y", "-l", "0", "-q", "160", "-k", "12", "-w", "5", "-I", "4G", "-p", "160", "-t", "4"]
    outs = [str(tmp_path / "s0.tsv"), str(tmp_path / "s1.tsv")]
    eng = _engine(gpu_lib, argv)
    eng.run_files_sets(target, [main_fq, short_fq], [160, 140], [160, 160], outs, err=str(tmp_path / "e"))
    eng.close()
    sep = []
    for fq, p in ((main_fq, "160"), (short_fq, "140")):
        eng = _engine(gpu_lib, argv[:-4] + ["-p", p, "-t", "4"])
        o = str(tmp_path / ("sep_%s.tsv" % p))
        eng.run_files(target, fq, out=o, err=str(tmp_path / "e2"))
        eng.close()
        sep.append(open(o).read())
    assert len(sep[0].splitlines()) == 4000 and len(sep[1].splitlines()) == 1000
    assert open(outs[0]).read() == sep[0]
    assert open(outs[1]).read() == sep[1]
    del synth


def synth_query_sets(d, n_main=4000, n_short=1000, seed=11):
    """configs[1]-shaped files (longqc_amd/synth.py): the targets, a seed-7 subsample of n_main reads and n_short pieces of
    200-499 bases cut from target reads -> (main.fq, short.fq, all.fq)"""
    from longqc_amd import synth
    cfg = synth.CONFIGS["cfg2"]
    T = synth.make_reads(cfg, synth.make_genome(cfg))
    Q = T.subset(synth.reservoir_subsample(len(T), n_main))
    rng = np.random.default_rng(seed)
    names, seqs, quals = [], [], []
    for j, i in enumerate(rng.choice(len(T), size=n_short, replace=False)):
        s, q = T.seqs[int(i)], T.quals[int(i)]
        L = int(rng.integers(200, 500))
        a = int(rng.integers(0, max(1, s.shape[0] - L)))
        names.append("short%d_%s" % (j, T.names[int(i)])); seqs.append(s[a:a + L]); quals.append(q[a:a + L])
    S = synth.ReadSet(names, seqs, quals)
    paths = [os.path.join(d, "main.fq"), os.path.join(d, "short.fq"), os.path.join(d, "all.fq")]
    synth.write_fastq(paths[0], Q); synth.write_fastq(paths[1], S); synth.write_fastq(paths[2], T)
    return paths


@pytest.mark.gpu
def test_gpu_saturated_counters_in_the_second_set(gpu_lib, tmp_path, monkeypatch):
    """set 1 holds the pile-up query whose narrowed (5-bit) counters saturate, at a -q of its own: the replayed row (the query's
    kept chains re-chained with its own `good` threshold and replayed in the reference's order) equals a separate run's"""
    from tests.test_emu_pipeline import _pileup_dataset
    tf, qf = _pileup_dataset(tmp_path, 300)
    monkeypatch.setenv("LQCOV_TEST_CNT_BITS", "5")
    base = ["-Y", "-l", "0", "-k", "12", "-w", "5", "-I", "4G", "-m", "20", "-t", "4"]
    other = str(tmp_path / "other.fq")
    _write_fastq(other, *[x[:4] for x in read_fastx(os.path.join(GOLDEN, "tiny_sub.fq.gz"))])
    qa = str(tmp_path / "pile.fq")
    names, seqs, _ = read_fastx(qf)
    _write_fastq(qa, names, seqs, [np.full(s.shape[0], ord("5"), np.uint8) for s in seqs])
    outs = [str(tmp_path / "s0.tsv"), str(tmp_path / "s1.tsv")]
    eng = _engine(gpu_lib, base + ["-p", "40", "-q", "40"])
    eng.run_files_sets(tf, [other, qa], [40, 40], [40, 60], outs, err=str(tmp_path / "e"))
    eng.close()
    assert "chains replayed" in open(str(tmp_path / "e")).read()
    sep = []
    for fq, q in ((other, "40"), (qa, "60")):
        eng = _engine(gpu_lib, base + ["-p", "40", "-q", q])
        o = str(tmp_path / ("sep%s.tsv" % q))
        eng.run_files(tf, fq, out=o, err=str(tmp_path / ("e" + q)))
        eng.close()
        sep.append(open(o).read())
    assert "chains replayed" in open(str(tmp_path / "e60")).read()
    assert open(outs[0]).read() == sep[0]
    assert open(outs[1]).read() == sep[1]
    monkeypatch.setenv("LQO_CNT_BITS", "5")
    assert sep[1] == oracle_bind.table(base + ["-p", "40", "-q", "60", tf, qa])

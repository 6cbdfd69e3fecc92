import ctypes as C
import os
import tempfile
from typing import List, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# Tests that take a good part of a minute each on the test emulator (every wave collective is 64 fiber switches; the default path
# runs two passes) or on three gloo ranks.  Each has a twin in tests/test_gpu_parity.py (the same check through the real library,
# `-m gpu`) or a smaller sibling that stays in the default run; LQCOV_SLOW_TESTS=1 runs them here too.
import pytest  # noqa: E402
slow_emu = pytest.mark.skipif(os.environ.get("LQCOV_SLOW_TESTS") != "1", reason="slow on the CPU test emulator; its GPU twin runs in -m gpu (LQCOV_SLOW_TESTS=1 runs it here)")

ONT = ["-Y", "-l", "0", "-q", "160", "-k", "12", "-w", "5", "-I", "4G", "-p", "160", "-t", "4"]


def run_main(lib, argv: List[str], cwd: Optional[str] = None):
    """lqcov_main through ctypes -> (rc, stdout table, stderr log)."""
    full = [b"minimap2-coverage"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(full))(*full)
    old = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        out, err = os.path.join(d, "o"), os.path.join(d, "e")
        try:
            if cwd:
                os.chdir(cwd)
            rc = lib.lqcov_main(len(full), arr, out.encode(), err.encode(), 0)
        finally:
            os.chdir(old)
        return rc, (open(out).read() if os.path.exists(out) else ""), (open(err).read() if os.path.exists(err) else "")


def parse_sketch_dump(text: str):
    """ref_harness / oracle `sketch` dump -> list of (name, len, [(x,y)...])"""
    reads = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "R":
            reads.append((f[1], int(f[2]), []))
        elif f[0] == "M":
            reads[-1][2].append((int(f[1], 16), int(f[2], 16)))
    return reads


def parse_chain_dump(text: str):
    """`chains` dump -> (mid_occ, {query index: dict(name, qlen, lambda, lambda2, chains=set(...), ivl=sorted, cnt={idx:n})})"""
    mid = None
    qs = {}
    cur = None
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "I":
            mid = int(f[2])
        elif f[0] == "Q":
            cur = dict(name=f[2], qlen=int(f[3]), n_regs=int(f[4]), lambda_=int(f[5]), lambda2=int(f[6]), chains=[], ivl=[], cnt={})
            qs[int(f[1])] = cur
        elif f[0] == "C":
            cur["chains"].append(tuple(int(x) for x in f[1:9]))
        elif f[0] == "V":
            cur["ivl"].append((int(f[1]), int(f[2])))
        elif f[0] == "N":
            cur["cnt"][int(f[1])] = int(f[2])
    return mid, qs


def read_fastx(path):
    """minimal FASTA/Q reader for tests (names, uint8 seq arrays, qual arrays or None)"""
    import gzip
    op = gzip.open if path.endswith(".gz") else open
    names, seqs, quals = [], [], []
    with op(path, "rb") as f:
        data = f.read().replace(b"\r\n", b"\n").split(b"\n")
    i = 0
    while i < len(data):
        l = data[i]
        if l.startswith(b"@"):
            names.append(l[1:].split()[0].decode()); seqs.append(np.frombuffer(data[i + 1], dtype=np.uint8)); quals.append(np.frombuffer(data[i + 3], dtype=np.uint8)); i += 4
        elif l.startswith(b">"):
            j = i + 1; parts = []
            while j < len(data) and not data[j].startswith(b">"):
                parts.append(data[j]); j += 1
            names.append(l[1:].split()[0].decode()); seqs.append(np.frombuffer(b"".join(parts), dtype=np.uint8)); quals.append(None); i = j
        else:
            i += 1
    return names, seqs, (quals if all(q is not None for q in quals) else None)


def limits_dataset(d, seed=0, glen=12000, n_targets=20, n_queries=5, err=0.02, n_noisy=3, n_indel=10):
    """the seeded repeat-rich set of tests/test_chain_limits.py (its docstring has the recipe), written to d -> (targets path, queries path)"""
    from longqc_amd import synth
    rng = np.random.default_rng(4100 + seed)
    A, COMP = synth._ACGT, synth._COMP
    g = A[rng.integers(0, 4, size=glen, dtype=np.uint8)]
    for at in range(500, glen - 3000, 2000):                    # tandem repeats
        u = int(rng.integers(40, 300)); c = min(int(rng.integers(4, 10)), 1800 // u)
        unit = g[at:at + u].copy()
        for i in range(c):
            g[at + i * u:at + (i + 1) * u] = synth._mutate(unit, rng, 0.01, (1, 0, 0))[:u]
    seg = g[1200:1700].copy()                                   # three dispersed copies of one segment
    g[5100:5600] = seg
    g[glen - 1500:glen - 1000] = COMP[seg[::-1]]

    def cut(st, L, e=err, flip=None):
        s = g[st:st + L]
        if flip if flip is not None else rng.random() < 0.5:
            s = COMP[s[::-1]]
        return synth._mutate(s, rng, e, (3, 3, 4))

    tseqs = [cut(int(rng.integers(0, glen - 4000)), int(rng.integers(1000, 4000))) for _ in range(n_targets - 1)]
    tseqs.append(cut(3000, 6500, 0.005, False))                 # the long pair
    qseqs = [cut(int(rng.integers(0, glen - 4000)), int(rng.integers(1500, 4000))) for _ in range(n_queries - 1)]
    qseqs.append(cut(2800, 6800, 0.005, False))
    for _ in range(n_noisy):                                    # sparse anchors: a predecessor exactly max_gap away can be the best one
        qseqs.append(cut(int(rng.integers(0, glen - 4000)), int(rng.integers(2000, 3000)), 0.13))
    for i in range(n_indel):                                    # exact copies of 400 bases with 20-24 more beyond a deletion of 70-97: two or three anchors 70-97 diagonals away
        a, dele, tail = 3300 + 550 * i, 70 + 3 * i, 20 + i % 5
        tseqs.append(np.concatenate([g[a:a + 400], g[a + 400 + dele:a + 400 + dele + tail]] if i % 2 == 0 else [g[a - dele - tail:a - dele], g[a:a + 400]]))

    def readset(prefix, seqs):
        return synth.ReadSet(["%s%03d" % (prefix, i) for i in range(len(seqs))], seqs, [(33 + rng.integers(3, 30, size=x.shape[0])).astype(np.uint8) for x in seqs])
    tf, qf = os.path.join(str(d), "lim_all.fq"), os.path.join(str(d), "lim_sub.fq")
    synth.write_fastq(tf, readset("t", tseqs)); synth.write_fastq(qf, readset("q", qseqs))
    return tf, qf


def seed_filter_dataset(d, seed=0, n_long=30, n_short=120):
    """the set of tests/test_seed_filter.py -> (target names, target reads, query names, query reads): limits_dataset (overlaps
    on both strands, tandem repeats) without its query of 6.8 kb, plus unrelated random targets -- n_long of 1.5-3.5 kb, whose
    chance hits with -k 9 fall several to a pair and spread over its diagonals, and n_short of 300-900 bases, a good third of
    whose pairs hold exactly one chance hit -- and copies of two queries under their own names (the self diagonal of -Y).  Half
    of the random reads are named to sort below the queries, half above (-X)."""
    from longqc_amd import synth
    tf, qf = limits_dataset(d, seed=seed)
    tn, ts, _ = read_fastx(tf)
    qn, qs, _ = read_fastx(qf)
    del qn[4], qs[4]                                            # (the long pair's query: one pair of thousands of hits)
    rng = np.random.default_rng(7300 + seed)
    for i in range(n_long + n_short):
        L = int(rng.integers(1500, 3500)) if i < n_long else int(rng.integers(300, 900))
        tn.append("%s%03d" % ("a" if i % 2 else "u", i)); ts.append(synth._ACGT[rng.integers(0, 4, size=L, dtype=np.uint8)])
    for i in (0, 4):
        tn.append(qn[i]); ts.append(qs[i].copy())
    return tn, ts, qn, qs


def seed_filter_long_pair(seed=0, L=9000):
    """a target and a query of about 9 kb that overlap at 6 % errors, under eight unrelated targets of 1.2 kb and two unrelated
    queries of 2 kb: with bw 0 the long pair's diagonals take more than 8192 bins of two, and the histograms of all the other
    pairs of a query still fit one bucket's space -> (target names, target reads, query names, query reads)"""
    from longqc_amd import synth
    rng = np.random.default_rng(7400 + seed)
    rnd = lambda n: synth._ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]
    g = rnd(L + 600)
    ts = [synth._mutate(g[:L], rng, 0.06, (3, 3, 4))] + [rnd(1200) for _ in range(8)]
    qs = [synth._mutate(g[600:], rng, 0.06, (3, 3, 4)), rnd(2000), rnd(2000)]
    return ["t%03d" % i for i in range(len(ts))], ts, ["q%03d" % i for i in range(len(qs))], qs


def all_hits(qxy, qoff, txy, qlen, qnames, tnames, mid_occ):
    """every occurrence in the part of every query minimizer whose list is shorter than mid_occ (lqmap.c:166-173), as columns:
    q (caller's order), rid, rs, diag, jl, y (query coordinate, lqmap.c:190-197), r (target position), drop_self (the self
    diagonal of -Y) and drop_ava (with -X: the targets named below the query), both lqmap.c:180-187"""
    qxy = qxy.astype(np.uint64); txy = txy.astype(np.uint64)
    qoff = qoff.astype(np.int64)
    tkey, ty = txy[:, 0] >> np.uint64(8), txy[:, 1]
    order = np.lexsort((ty, tkey))
    tkey, ty = tkey[order], ty[order]
    qkey = qxy[:, 0] >> np.uint64(8)
    lo, hi = np.searchsorted(tkey, qkey, "left"), np.searchsorted(tkey, qkey, "right")
    n = hi - lo
    n = np.where(n < mid_occ, n, 0)
    j = np.repeat(np.arange(qkey.shape[0], dtype=np.int64), n)                        # the hit's query minimizer
    at = lo[j] + (np.arange(j.shape[0], dtype=np.int64) - np.repeat(np.cumsum(n) - n, n))
    occ = ty[at]
    q = np.searchsorted(qoff, j, "right") - 1
    rid = (occ >> np.uint64(32)).astype(np.int64)
    rpos = ((occ & np.uint64(0xffffffff)) >> np.uint64(1)).astype(np.int64)
    qy = qxy[j, 1]
    qpos = ((qy & np.uint64(0xffffffff)) >> np.uint64(1)).astype(np.int64)
    span = (qxy[j, 0] & np.uint64(0xff)).astype(np.int64)
    rs = ((occ ^ qy) & np.uint64(1)).astype(np.int64)
    ql = np.asarray(qlen, dtype=np.int64)[q]
    y = np.where(rs == 1, ql - (qpos + 1 - span) - 1, qpos)
    diag = rpos - y + ql + 256
    same = np.array([[qn == tn for tn in tnames] for qn in qnames])
    below = np.array([[tn.encode() < qn.encode() for tn in tnames] for qn in qnames])
    return dict(q=q, rid=rid, rs=rs, diag=diag, jl=j - qoff[q], y=y.astype(np.int32), r=rpos.astype(np.int32),
                drop_self=same[q, rid] & (rpos == qpos), drop_ava=below[q, rid])


# ---- tests/test_intervals.py: overlap intervals of the test's choosing, as text for `ref_harness intervals` ----
IVL_N_QUERIES = 130                                             # 64 + 64 + 2 threads of k_filter_redundant / k_reliable
# queries (caller's order) without any interval.  The engine holds the queries longest first, the test runs every case with the
# lengths ascending and descending: the set is its own mirror image at the ends and in the middle, so that the engine's
# positions 0, 63, 64 and 129 (the edges of the 64-thread blocks) are empty both times; 17 and 100 lie inside a block
IVL_EMPTY = (0, 17, 63, 64, 65, 66, 100, 129)


def ivl_enc(s, e, med):
    """a chain's query interval [s, e) as esterr.c:122-125 encodes it: position << 3 | 2 if the score is medium | 1 at the end"""
    f = 2 if med else 0
    return (s << 3) | f, (e << 3) | f | 1


def _ivl_random(rng, n, span, lengths, p_med=0.6):
    out = []
    for _ in range(n):
        L = int(lengths[int(rng.integers(0, len(lengths)))]) if isinstance(lengths, (list, tuple)) else int(rng.integers(lengths.start, lengths.stop))
        s = int(rng.integers(0, span - L + 1))
        out.append(ivl_enc(s, s + L, bool(rng.random() < p_med)))
    return out


def _ivl_quirk_block(form):
    """lqmap.c:63 takes the decoded end minus the *encoded* start: a merged region that closes where end == 8 * start + 2 (the
    start event of a medium interval carries flag 2) has length 0 there and makes no marker.  form 1 (for -c 1): a lone medium
    interval [s, 8s + 2); form 2 (for -c 2): [max(s - 1, 0), 8s + 2) under [s, 8s + 5), the coverage reaches 2 at s and leaves it
    at 8s + 2.  With each, the neighbours that close one base earlier and later.  -> [(s, offset of the end, [intervals])] * 12"""
    out = []
    for s in range(4):
        for d in (-1, 0, 1):
            x = 8 * s + 2 + d
            out.append((s, d, [ivl_enc(s, x, True)] if form == 1 else [ivl_enc(max(s - 1, 0), x, True), ivl_enc(s, 8 * s + 5, True)]))
    return out


def _ivl_marker_block(min_cov):
    """part 0: min_cov medium intervals [100, 200), which the filter merges into one marker; part 1: an interval strictly inside
    the merged region, equal to it, sharing one end with it, overhanging it by one base on either side or both -- each as one
    medium interval, as one that is not medium, and as min_cov medium ones (a second merged region); part 2: one medium interval
    over everything.  -> [[part 0, part 1, part 2]] * 21, one entry per query"""
    out = []
    for s, e in ((120, 150), (100, 200), (100, 150), (150, 200), (99, 200), (100, 201), (99, 201)):
        for med, copies in ((True, 1), (False, 1), (True, min_cov)):
            out.append([[ivl_enc(100, 200, True)] * min_cov, [ivl_enc(s, e, med)] * copies, [ivl_enc(50, 250, True)]])
    return out


def make_interval_cases(seed=83):
    """The generator of the inputs of tests/test_intervals.py (its docstring describes them): a list of dict(name, min_cov, parts =
    three lists of (query in the caller's order, start, end) in the order the reference is given them, quirk = {query: (form, s,
    offset)} for the hand-made inputs of lqmap.c:63, whose intervals are all in part 0, random = the queries whose intervals are
    the same in every `mixed` case, grows = the part whose call has to move the persisted intervals to a larger pool, or None).
    What it made is kept under tests/golden/intervals/ (tests/golden/make_interval_inputs.py): the recorded runs of the reference
    are keyed by the bytes of their input, which must not hang on a random generator's stream staying what it was."""
    rng = np.random.default_rng(seed)
    usable = [q for q in range(IVL_N_QUERIES) if q not in IVL_EMPTY]
    slots = [usable[i] for i in rng.permutation(len(usable))]
    fam = {}
    for name, n in (("crowded12", 8), ("crowded40", 8), ("ord3000", 2), ("ord200000", 2), ("marker", 21), ("quirk1", 12), ("quirk2", 12)):
        fam[name], slots = slots[:n], slots[n:]
    fam["sparse"] = slots
    rnd = [[], [], []]                                          # the same in every mixed case
    for p in range(3):
        for q in fam["crowded12"] + fam["crowded40"]:
            span = 12 if q in fam["crowded12"] else 40
            rnd[p] += [(q,) + iv for iv in _ivl_random(rng, int(rng.integers(6, 41)), span, [0, 1, 2, span // 8, span // 2])]
        for q in fam["ord3000"] + fam["ord200000"]:
            span = 3000 if q in fam["ord3000"] else 200000
            rnd[p] += [(q,) + iv for iv in _ivl_random(rng, int(rng.integers(30, 65)), span, range(span // 50, span // 3))]
        for q in fam["sparse"]:
            rnd[p] += [(q,) + iv for iv in _ivl_random(rng, int(rng.integers(0, 3)), 3000, range(50, 1500))]
    random_queries = sorted(fam["crowded12"] + fam["crowded40"] + fam["ord3000"] + fam["ord200000"] + fam["sparse"])
    cases = []
    for c in (1, 2, 3, 5):
        parts = [list(x) for x in rnd]
        quirk = {}
        for form in (1, 2):
            for q, (s, d, ivs) in zip(fam["quirk%d" % form], _ivl_quirk_block(form)):
                parts[0] += [(q,) + iv for iv in ivs]
                quirk[q] = (form, s, d)
        for q, per_part in zip(fam["marker"], _ivl_marker_block(c)):
            for p in range(3):
                parts[p] += [(q,) + iv for iv in per_part[p]]
        parts = [[ivs[i] for i in rng.permutation(len(ivs))] for ivs in parts]   # (the queries' lines interleaved)
        cases.append(dict(name="mixed_c%d" % c, min_cov=c, parts=parts, quirk=quirk, random=random_queries, grows=None))
    # the long list: a query of 1800 intervals a part (the per-thread heapsort over 3600 and, in pass 2, over all that is persisted)
    # between neighbours of one and of two intervals, and a query whose intervals are all the same
    parts = []
    for p in range(3):
        one = [(70,) + iv for iv in _ivl_random(rng, 1800, 3000000, range(200, 10000))]
        one += [(69,) + iv for iv in _ivl_random(rng, 1, 3000000, range(200, 10000))] + [(71,) + iv for iv in _ivl_random(rng, 2, 3000000, range(200, 10000))]
        one += [(40,) + ivl_enc(1000, 2000, True)] * 30
        parts.append([one[i] for i in rng.permutation(len(one))])
    cases.append(dict(name="long_c3", min_cov=3, parts=parts, quirk={}, random=[], grows=None))
    # growth: a small first part leaves a small pool with intervals in it, the second part does not fit
    qs = [q for q in usable if q % 3 == 0]
    parts = [[(qs[int(rng.integers(0, 5))],) + iv for iv in _ivl_random(rng, 12, 300, range(20, 200), 1.0)],
             [(qs[int(rng.integers(0, len(qs)))],) + iv for iv in _ivl_random(rng, 300, 3000, range(50, 1500))],
             [(qs[int(rng.integers(0, len(qs)))],) + iv for iv in _ivl_random(rng, 20, 3000, range(50, 1500))]]
    cases.append(dict(name="growth_c3", min_cov=3, parts=parts, quirk={}, random=[], grows=1))
    return cases


def interval_cases():
    """the inputs of tests/test_intervals.py as committed: tests/golden/intervals/cases.json (name, min_cov, quirk, random, grows
    of every case) and <name>.txt.gz (its intervals, as the text the harness reads) -> the list make_interval_cases describes"""
    import gzip
    import json
    d = os.path.join(GOLDEN, "intervals")
    cases = json.load(open(os.path.join(d, "cases.json")))
    for c in cases:
        c["quirk"] = {int(q): tuple(v) for q, v in c["quirk"].items()}
        with gzip.open(os.path.join(d, c["name"] + ".txt.gz"), "rt") as f:
            head = f.readline().split()
            assert head[0] == "H" and int(head[1]) == IVL_N_QUERIES
            c["parts"] = [[] for _ in range(int(head[2]))]
            for line in f:
                t = line.split()
                c["parts"][int(t[1])].append((int(t[2]), int(t[3]), int(t[4])))
    return cases


def write_interval_case(case, path):
    """a case as the text `ref_harness intervals` and `lqcov_oracle intervals` read"""
    with open(path, "w") as f:
        f.write("H %d %d\n" % (IVL_N_QUERIES, len(case["parts"])))
        for p, ivs in enumerate(case["parts"]):
            for q, s, e in ivs:
                f.write("I %d %d %d %d\n" % (p, q, s, e))


def parse_interval_dump(text, n_parts=3):
    """`intervals` dump -> (V[part][query] = sorted [(start, end)], R[query] = [(start, end)] as pushed, M[query] likewise)"""
    V = [dict() for _ in range(n_parts)]
    R, M = {}, {}
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "V":
            V[int(f[1])].setdefault(int(f[2]), []).append((int(f[3]), int(f[4])))
        elif f[0] in ("R", "M"):
            (R if f[0] == "R" else M).setdefault(int(f[1]), []).append((int(f[2]), int(f[3])))
    return V, R, M

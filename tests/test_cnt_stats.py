"""k_cnt_stats (kernels_chain.hpp; finish() in engine.cpp): the n_match column -- minimap2-coverage.c:552-561, the integer mean of a
query's match counters and the number of counters above it -- and the two flags it raises, at its own stage.

One wave works on a query, its lanes striding over the counters, and the partial sums meet through shuffles.  What can go wrong
there and nowhere else: a query with fewer counters than lanes, one with exactly 64, one counter more than a whole number of
strides, a sum that passes 2^32 (the reference adds into a uint32_t: the sum wraps, whatever the order of the additions), the
division left out for a query without counters, a flag seen by one lane and lost on the way to the lane that stores it.

The way in: lqcov_accum_import_dev puts counters of the test's choosing into the handle (the call a rank of a multi-GPU run
merges the other ranks' counters with), finish() runs k_cnt_stats over them, rows() gives n_match and the flags back.  The
model is the reference's loop in numpy.  Queries: prefixes of one random sequence chosen so that they have 0, 1, 63, 64, 65 and
129 minimizers, one read of some thousand and one of more than 65 537 (the shortest whose counters can add up to 2^32 with 16-bit
counters: that pattern is reachable, so it is not skipped).  Patterns: all counters equal (nothing above the mean); one above the
mean; random ones; all at 65 534 (the long read's sum wraps, nothing saturates); some at the limit (LQCOV_ROW_SATURATED on those
queries alone); and, with LQCOV_TEST_CNT_BITS=5, counters at and beyond 31.

Not covered: the layout after lqcov_handle::adopt_index_params (`nsize`: counters the reference never allocated, flag 2).  The
import copies as many counters as the queries have minimizers under the index's parameters, which is not that layout's size, and
no other hook writes counters: tests/test_mmi.py reaches the layout through whole runs."""
import numpy as np
import pytest

from longqc_amd import api

K, W = 12, 5
SIZES = [0, 1, 63, 64, 65, 129]
SATURATED = 1                                                   # LQCOV_ROW_SATURATED
_QUERIES = {}


def params(lib):
    p = api.Params()
    lib.lqcov_params_default(p)
    p.k, p.w = K, W
    return p


def counts_of(lib, seqs):
    """minimizers per query, in the caller's order"""
    eng = api.Engine(params(lib), 0, lib=lib)
    try:
        eng.set_queries(["c%d" % i for i in range(len(seqs))], seqs)
        _, off = eng.query_minimizers()
    finally:
        eng.close()
    return np.diff(off.astype(np.int64))


def queries(lib):
    """the test's queries, made once: (names, sequences, minimizers of each)"""
    if not _QUERIES:
        rng = np.random.default_rng(552)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        base = acgt[rng.integers(0, 4, size=700)]
        lens = list(range(K - 2, base.shape[0]))
        cnt = counts_of(lib, [base[:n] for n in lens])
        seqs = []
        for want in SIZES:
            hit = np.flatnonzero(cnt == want)
            assert hit.shape[0], "no prefix with %d minimizers" % want
            seqs.append(base[:lens[int(hit[0])]])
        seqs.append(acgt[rng.integers(0, 4, size=9000)])
        seqs.append(acgt[rng.integers(0, 4, size=230000)])
        n = counts_of(lib, seqs)
        assert n[:len(SIZES)].tolist() == SIZES and 2000 < n[-2] < 65536 and n[-1] > 65537, n
        _QUERIES["q"] = (["q%d" % i for i in range(len(seqs))], seqs, n)
    return _QUERIES["q"]


def model(raw, cnt_max):
    """minimap2-coverage.c:552-561 on one query's counters -> (n_match, saturated)"""
    c = raw & np.uint32(cnt_max)
    s = int(c.astype(np.uint64).sum()) & 0xffffffff             # uint32_t sum
    if c.shape[0]:
        s //= c.shape[0]
    return int(np.sum(c > s)), bool(np.any(raw >= cnt_max))


def patterns(n, cnt_max, rng):
    """name -> the counters of every query (caller's order), n: their numbers"""
    out = {}
    out["all_equal"] = [np.full(m, 7, dtype=np.uint32) for m in n]
    one = [np.full(m, 3, dtype=np.uint32) for m in n]
    for i, c in enumerate(one):
        if c.shape[0]:
            c[(c.shape[0] * (i + 1)) // (len(n) + 1)] = 9      # (a different lane in every query)
    out["one_above"] = one
    out["random"] = [rng.integers(0, min(cnt_max, 200), size=m, dtype=np.uint32) for m in n]
    out["below_the_limit"] = [np.full(m, cnt_max - 1, dtype=np.uint32) for m in n]
    lim = [rng.integers(0, 5, size=m, dtype=np.uint32) for m in n]
    for i, c in enumerate(lim):
        if i % 2 == 1 and c.shape[0]:
            c[c.shape[0] - 1] = cnt_max                         # the limit itself, in the last counter: one lane sees it
        if i == 4:
            c[0] = cnt_max + 9                                  # beyond it (a merged sum): counted as its low bits
    out["at_the_limit"] = lim
    return out


def run(lib, on_device, cnt_bits, monkeypatch):
    names, seqs, n = queries(lib)
    if cnt_bits:
        monkeypatch.setenv("LQCOV_TEST_CNT_BITS", str(cnt_bits))
    else:
        monkeypatch.delenv("LQCOV_TEST_CNT_BITS", raising=False)
    cnt_max = (1 << (cnt_bits or 16)) - 1
    rng = np.random.default_rng(561 + cnt_bits)
    pats = patterns(n, cnt_max, rng)
    if not cnt_bits:                                            # the sum this pattern is for does pass 2^32
        assert int(n[-1]) * (cnt_max - 1) > 1 << 32
    eng = api.Engine(params(lib), 0, lib=lib)
    try:
        eng.set_queries(names, seqs)
        perm = eng.query_order().astype(np.int64)               # perm[i]: the caller's index of the engine's i-th query
        n_q, n_cnt, _ = eng.accum_sizes()
        assert n_q == len(seqs) and n_cnt == int(n.sum())
        for name, per_query in pats.items():
            flat = np.concatenate([per_query[j] for j in perm]).astype(np.uint32)
            arrs = [np.zeros(n_q, dtype=np.uint64), np.zeros(n_q, dtype=np.uint64), np.zeros(n_q, dtype=np.float32), np.zeros(n_q, dtype=np.uint32),
                    flat, np.zeros(3, dtype=np.uint32)]
            if on_device:                                       # the real library copies device to device
                import torch
                keep = [torch.from_numpy(a.view(np.uint8)).to("cuda:0") for a in arrs]
                ptrs = [t.data_ptr() for t in keep]
            else:                                               # the emulator's device memory is the host's
                ptrs = [a.ctypes.data for a in arrs]
            eng.accum_import(*ptrs, 0)
            eng.finish()
            rows = eng.rows()
            for j, r in enumerate(rows):
                want_nm, want_sat = model(per_query[j], cnt_max)
                assert r["n_mini"] == n[j]
                assert r["n_match"] == want_nm, "%s, query of %d counters: n_match %d, the model has %d" % (name, n[j], r["n_match"], want_nm)
                assert r["flags"] == (SATURATED if want_sat else 0), "%s, query of %d counters: flags %d, saturated in the model: %s" % (name, n[j], r["flags"], want_sat)
            if name == "all_equal":
                assert all(r["n_match"] == 0 for r in rows)
            if name == "one_above":
                assert [r["n_match"] for r in rows] == [0, 0] + [1] * (len(rows) - 2)
            if name == "at_the_limit":
                assert [r["flags"] for r in rows] == [SATURATED if (j % 2 == 1 or j == 4) else 0 for j in range(len(rows))]
    finally:
        eng.close()


@pytest.mark.parametrize("cnt_bits", [0, 5])
def test_emulated_cnt_stats_is_the_references_loop(emu_lib, cnt_bits, monkeypatch):
    run(emu_lib, False, cnt_bits, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("cnt_bits", [0, 5])
def test_gpu_cnt_stats_is_the_references_loop(gpu_lib, cnt_bits, monkeypatch):
    run(gpu_lib, True, cnt_bits, monkeypatch)

"""The mapping stage's host decisions alone (longqc_amd/csrc/mapplan.hpp), without a handle, a device or the emulator: the header
is compiled with g++ behind tests/emu/mapplan_shim.cpp and fed offsets made up here.  Expected values are either a plain model
of the rule written below from the header's comments, or literals recorded from the parent commit's inline code (a throw-away
program around the pasted lines of map_part and seed_filter) before it moved; never what the shim itself answers.

The batch cut aims at a count that is a multiple of the lane count and then cuts greedily, query by query: with queries of
one size the cuts are exact and the count is the one aimed at; with uneven queries a cut may fall short of its share and one
more batch follows (recorded from the parent: 4 batches for 3 lanes, CUT_RECORDED below).  So "a multiple of the lane count
whenever it exceeds it" is asserted where every query has one size, and the uneven cases are pinned to the parent's batches."""
import ctypes as C
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "emu", "mapplan_shim.cpp")
RS_MIN, SL_SMALL, SL_BIG = 64, 512, 2048          # lq_common.hpp (ksort.h:81), seed_geom.hpp
U32 = 0xffffffff


class ShimError(Exception):
    pass


def build(out, *flags):
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, SRC, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mapplan_shim") / "mapplan_shim.so")
    build(so, "-shared", "-fPIC")
    lib = C.CDLL(so)
    lib.shim_mapplan.restype = C.c_longlong
    lib.shim_mapplan.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]

    def call(name, words, cap=1 << 16):
        a = (C.c_uint64 * max(len(words), 1))(*words)
        out = (C.c_uint64 * cap)()
        err = C.create_string_buffer(256)
        n = lib.shim_mapplan(name.encode(), a, len(words), out, cap, err, 256)
        if n < 0:
            raise ShimError(err.value.decode())
        return list(out[:n])
    return call


# ---- the batch cut ------------------------------------------------------------------------------------------------------------
def cut_words(off, h_aq, g_begin, g_end, budget, lanes):
    assert len(off) == len(h_aq)
    return [lanes, budget, g_begin, g_end, len(off)] + list(off) + list(h_aq)


def cut(shim, *a):
    w = shim("cut", cut_words(*a))
    assert len(w) == 1 + 2 * w[0]
    return [(w[1 + 2 * i], w[2 + 2 * i]) for i in range(w[0])]


def cut_model(off, h_aq, g_begin, g_end, budget, lanes):
    """As few batches as the budget allows; at least one per lane when the group's seed hits reach lanes << 24; more than the
    lanes: rounded up to a multiple of them; then batch by batch an equal share of what is left, never above the budget, at
    least one query."""
    nb = -(-(off[g_end] - off[g_begin]) // budget)
    if nb < lanes and h_aq[g_end] - h_aq[g_begin] >= lanes << 24:
        nb = lanes
    if nb > lanes:
        nb = -(-nb // lanes) * lanes
    left, out, q0 = max(nb, 1), [], g_begin
    while q0 < g_end:
        rem = off[g_end] - off[q0]
        lim = min(budget, -(-rem // left) if left > 1 else rem)
        q1 = q0 + 1
        while q1 < g_end and off[q1 + 1] - off[q0] <= lim:
            q1 += 1
        out.append((q0, q1))
        q0, left = q1, max(left - 1, 1)
    return out


def cut_properties(batches, off, g_begin, g_end, budget, lanes, even):
    assert batches[0][0] == g_begin and batches[-1][1] == g_end
    for (a0, a1), (b0, _) in zip(batches, batches[1:]):
        assert a1 == b0                                     # they tile the group in order
    for q0, q1 in batches:
        assert q1 > q0                                      # none is empty
        assert off[q1] - off[q0] <= budget or q1 == q0 + 1   # above the budget: a single query
    if even and len(batches) > lanes:
        assert len(batches) % lanes == 0


def offs(sizes):
    o = [0]
    for s in sizes:
        o.append(o[-1] + s)
    return o


B = 1000
CUT_CASES = [   # (name, sizes of `off`, sizes of h_aq or None for the same, g_begin, budget, queries of one size)
    ("total 0", [0, 0, 0, 0], None, 0, B, True),
    ("one query above the budget", [5, 3 * B, 5], None, 0, B, False),
    ("one query above the budget, alone", [3 * B], None, 0, B, True),
    ("exactly the budget", [1] * B, None, 0, B, True),
    ("the budget + 1", [1] * (B + 1), None, 0, B, True),
    ("begins in the middle", [7] * 400, None, 150, B, True),
]


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_batch_cut(shim, lanes):
    cases = CUT_CASES + [("lanes * budget + 1", [1] * (lanes * B + 1), None, 0, B, True)]
    for name, sizes, hits, g_begin, budget, even in cases:
        off = offs(sizes)
        h_aq = offs(hits) if hits else off
        got = cut(shim, off, h_aq, g_begin, len(sizes), budget, lanes)
        assert got == cut_model(off, h_aq, g_begin, len(sizes), budget, lanes), name
        cut_properties(got, off, g_begin, len(sizes), budget, lanes, even)
    assert cut(shim, offs([0] * 4), offs([0] * 4), 0, 4, B, lanes) == [(0, 4)]
    assert (1, 2) in cut(shim, offs([5, 3 * B, 5]), offs([5, 3 * B, 5]), 0, 3, B, lanes)          # its own batch
    assert len(cut(shim, offs([1] * B), offs([1] * B), 0, B, B, lanes)) == 1
    n = len(cut(shim, offs([1] * (B + 1)), offs([1] * (B + 1)), 0, B + 1, B, lanes))
    assert n == 2
    n = len(cut(shim, offs([1] * (lanes * B + 1)), offs([1] * (lanes * B + 1)), 0, lanes * B + 1, B, lanes))
    assert n == 2 * lanes                                   # lanes + 1 batches would do: rounded up to the next multiple


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_batch_cut_by_the_seed_hits(shim, lanes):
    """The survivors are few (one per query, far below the budget) but the group's seed hits reach lanes << 24: a batch per lane."""
    n = 6
    off = offs([1] * n)
    for total, want in (((lanes << 24) - 1, 1), (lanes << 24, lanes)):
        h_aq = offs([total // n] * (n - 1) + [total - total // n * (n - 1)])
        got = cut(shim, off, h_aq, 0, n, B, lanes)
        assert got == cut_model(off, h_aq, 0, n, B, lanes)
        assert len(got) == want
        cut_properties(got, off, 0, n, B, lanes, True)


# recorded from the parent's cut_batches: off = h_aqf, nine queries of uneven size, g_end = 9
CUT_AQ = [0, 100, 100, 5000, 5400, 6000, 9000, 9100, 9100, 12000]
CUT_AQF = [0, 10, 10, 900, 950, 1000, 1700, 1710, 1710, 2500]
SIX, FOUR = [(0, 2), (2, 3), (3, 5), (5, 6), (6, 8), (8, 9)], [(3, 5), (5, 6), (6, 8), (8, 9)]
CUT_RECORDED = {   # (lanes, budget, g_begin): batches
    (1, 400, 0): SIX, (1, 400, 3): FOUR, (1, 1000, 0): [(0, 2), (2, 5), (5, 8), (8, 9)], (1, 1000, 3): [(3, 6), (6, 9)],
    (2, 400, 0): SIX, (2, 400, 3): FOUR, (2, 1000, 0): [(0, 2), (2, 3), (3, 6), (6, 9)], (2, 1000, 3): [(3, 6), (6, 9)],
    (3, 400, 0): SIX, (3, 400, 3): FOUR, (3, 1000, 0): [(0, 2), (2, 5), (5, 8), (8, 9)], (3, 1000, 3): [(3, 6), (6, 9)],
}


def test_batch_cut_as_the_parent_cut(shim):
    for (lanes, budget, g_begin), want in CUT_RECORDED.items():
        got = cut(shim, CUT_AQF, CUT_AQ, g_begin, 9, budget, lanes)
        assert got == want == cut_model(CUT_AQF, CUT_AQ, g_begin, 9, budget, lanes)
        cut_properties(got, CUT_AQF, g_begin, 9, budget, lanes, False)


# ---- the second pass's subsets ------------------------------------------------------------------------------------------------
def subsets_words(want, h_aq, h_qmoff, budget):
    assert len(h_aq) == len(h_qmoff)
    return [budget, len(want), len(h_aq)] + list(want) + list(h_aq) + list(h_qmoff)


def subsets(shim, *a):
    w = shim("subsets", subsets_words(*a))
    want, w = w[1:1 + w[0]], w[1 + w[0]:]
    out, w = [], w[1:]
    while w:
        ns, mm = w[0], w[1]
        out.append((w[2:2 + ns], w[2 + ns:2 + 2 * ns], w[2 + 2 * ns:3 + 3 * ns], mm))
        w = w[3 + 3 * ns:]
    return want, out


def subsets_model(want, h_aq, h_qmoff, budget):
    """The keys sorted, each once; their queries in order; subsets filled while the seed hits fit the budget, a query above it
    alone; klib's passes for queries of more than 64 anchors; max_mini: the most minimizers of a query so far in the batch."""
    want = sorted(set(want))
    fq = sorted({k >> 32 for k in want})
    out, run_max = [], 0
    for qi in fq:
        ln = h_aq[qi + 1] - h_aq[qi]
        if not out or out[-1][2][-1] + ln > budget:
            out.append(([], [], [0], 0))
        sq, sk, so, _ = out[-1]
        sq.append(qi); sk.append(1 if ln > RS_MIN else 0); so.append(so[-1] + ln)
        run_max = max(run_max, h_qmoff[qi + 1] - h_qmoff[qi])
        out[-1] = (sq, sk, so, run_max)
    return want, out


def key(q, run):
    return q << 32 | run


SUBSET_CASES = [
    # duplicate keys, two runs of query 1, queries of 64 and 65 anchors, a query that owns no run in between
    ([key(1, 5), key(0, 2), key(1, 5), key(1, 9), key(3, 0)], offs([64, 65, 10, 100, 7]), offs([3, 8, 2, 4, 1]), 10 ** 6),
    # query 0 alone above the budget
    ([key(2, 1), key(0, 1), key(1, 1)], offs([500, 20, 30]), offs([9, 1, 2]), 100),
    # three subsets whose own maxima are 5, 9 and 2
    ([key(0, 0), key(1, 0), key(2, 0)], offs([80, 80, 80]), offs([5, 9, 2]), 100),
]


def test_second_pass_subsets(shim):
    for c in SUBSET_CASES:
        assert subsets(shim, *c) == subsets_model(*c)
    want, subs = subsets(shim, *SUBSET_CASES[0])
    assert want == [key(0, 2), key(1, 5), key(1, 9), key(3, 0)]
    assert subs == [([0, 1, 3], [0, 1, 1], [0, 64, 129, 229], 8)]
    _, subs = subsets(shim, *SUBSET_CASES[1])
    assert [(s[0], s[2]) for s in subs] == [([0], [0, 500]), ([1, 2], [0, 20, 50])]
    _, subs = subsets(shim, *SUBSET_CASES[2])
    assert [s[3] for s in subs] == [5, 9, 9]                # a running maximum: the grid of the subset's k_seed_emit


# ---- the seed filter's geometry -----------------------------------------------------------------------------------------------
def geometry_words(h_hq, h_qmoff, q_begin, q_stop, n_targets, bucket, segl, chunk, with_segs=1):
    assert len(h_hq) == len(h_qmoff)
    return [q_begin, q_stop, len(h_hq) - 1, n_targets, bucket, segl, chunk, with_segs] + list(h_hq) + list(h_qmoff)


def geometry(shim, *a, **kw):
    words = geometry_words(*a, **kw)
    n_q = words[2]
    w = shim("geometry", words)
    n_segs, n_bq, n_chunks = w[:3]
    g = dict(max=tuple(w[3:6]), sizes=tuple(w[6:8]))
    w = w[8:]
    g["qg"], w = [tuple(w[6 * i:6 * i + 6]) for i in range(n_q)], w[6 * n_q:]
    g["has"], w = w[:n_q], w[n_q:]
    g["bq"], w = w[:n_bq], w[n_bq:]
    g["chunks"], w = [tuple(w[10 * i:10 * i + 10]) for i in range(n_chunks)], w[10 * n_chunks:]
    g["segs"] = [tuple(w[4 * i:4 * i + 4]) for i in range(n_segs)] if words[7] else None
    assert len(w) == (4 * n_segs if words[7] else 0)
    return g


def geometry_model(h_hq, h_qmoff, q_begin, q_stop, n_targets, bucket, segl, chunk):
    """Per query with hits: about `bucket` hits per slice, at most SL_BIG slices and half the targets, at least one; mul =
    floor(2^32 nsl / targets) (0 for one slice); segments of segl minimizers.  Chunks: queries while the hits fit max(chunk,
    the largest query).  cb, bk: the running sums of pieces (slices x segments) and buckets (slices) inside the chunk."""
    n_q = len(h_hq) - 1
    cap = max(chunk, max(h_hq[i + 1] - h_hq[i] for i in range(n_q)))
    qg, has, bq, chunks, segs = [(0,) * 6] * n_q, [0] * n_q, [], [], []
    i = q_begin
    while i < q_stop:
        c = dict(q_lo=i, g_lo=len(segs), ne=0, nb=0, hits=0, h0=h_hq[i], big=0, bq_at=len(bq))
        while i < q_stop and (c["hits"] == 0 or c["hits"] + h_hq[i + 1] - h_hq[i] <= cap):
            hq, nm = h_hq[i + 1] - h_hq[i], h_qmoff[i + 1] - h_qmoff[i]
            mul = nsl = nseg = 0
            seg0, cb, bk = len(segs), c["ne"], c["nb"]
            if hq:
                has[i] = 1
                nsl = max(min(-(-hq // bucket), SL_BIG, max(n_targets // 2, 1)), 1)
                mul = 0 if nsl == 1 else (nsl << 32) // n_targets
                nseg = -(-nm // segl)
                segs += [(h_qmoff[i] + p * segl, min(h_qmoff[i] + (p + 1) * segl, h_qmoff[i + 1]), i, p) for p in range(nseg)]
                c["big"] |= int(nsl > SL_SMALL)
                c["ne"] += nsl * nseg; c["nb"] += nsl; c["hits"] += hq
            bq.append(bk)
            qg[i] = (mul, nsl, nseg, seg0, cb, bk)
            i += 1
        bq.append(c["nb"])
        chunks.append((c["q_lo"], i, c["g_lo"], len(segs), c["ne"], c["nb"], c["hits"], c["h0"], c["big"], c["bq_at"]))
    mx = tuple(max([c[k] for c in chunks], default=0) for k in (4, 5, 6))
    return dict(max=mx, sizes=(32, 32), qg=qg, has=has, bq=bq, chunks=chunks, segs=segs)


@pytest.mark.parametrize("n_targets", [1, 2, 3, 1023, 1024, 4097, 2 ** 31 - 1])
def test_seed_geometry_slices_of_targets(shim, n_targets):
    """One query whose hits ask for 1, 2, SL_SMALL, SL_SMALL + 1 and SL_BIG slices (and one more): slice(rid) = rid * mul >> 32
    is monotone, 0 at rid 0 and below nsl at the last rid; no more slices than half the targets."""
    bucket = 10
    for ask in (1, 2, SL_SMALL, SL_SMALL + 1, SL_BIG, SL_BIG + 1):
        a = ([0, ask * bucket], [0, 3], 0, 1, n_targets, bucket, 256, 1 << 30)
        g = geometry(shim, *a)
        assert g == geometry_model(*a)
        mul, nsl, nseg, seg0, cb, bk = g["qg"][0]
        assert nsl == max(min(ask, SL_BIG, n_targets // 2), 1) and nsl <= max(n_targets // 2, 1)
        assert mul <= U32 and (mul == 0) == (nsl == 1)
        sl = lambda rid: rid * mul >> 32
        assert sl(0) == 0 and sl(n_targets - 1) < nsl
        rids = sorted(r for r in {0, 1, 2, n_targets // 3, n_targets // 2, n_targets - 2, n_targets - 1} if 0 <= r < n_targets)
        assert [sl(r) for r in rids] == sorted(sl(r) for r in rids)
        if n_targets <= 4097:
            s = [sl(r) for r in range(n_targets)]
            assert s == sorted(s) and s[-1] < nsl
        assert g["chunks"][0][8] == int(nsl > SL_SMALL)     # big: the scatter kernel's other shape
        assert g["bq"] == [0, nsl] and g["max"] == (nsl * nseg, nsl, ask * bucket)


# recorded from the parent's seed_filter: LQCOV_SEED_BUCKET=100, LQCOV_SEED_SEGL=4, LQCOV_SEED_CHUNK=1000, seven targets, the group from
# query 1 on; query 2 has no hits, query 3 (1250 hits) is above the chunk and alone in it, query 3 has exactly segl minimizers
GEO_RECORDED = ([0, 50, 650, 650, 1900, 2000, 2300], [0, 3, 11, 15, 19, 20, 29], 1, 6, 7, 100, 4, 1000)
GEO_RECORDED_WANT = dict(
    qg=[(0, 0, 0, 0, 0, 0), (1840700269, 3, 2, 0, 0, 0), (0, 0, 0, 2, 6, 3), (1840700269, 3, 1, 2, 0, 0), (0, 1, 1, 3, 0, 0), (1840700269, 3, 3, 4, 1, 1)],
    has=[0, 1, 0, 1, 1, 1], bq=[0, 3, 3, 0, 3, 0, 1, 4],
    chunks=[(1, 3, 0, 2, 6, 3, 600, 50, 0, 0), (3, 4, 2, 3, 3, 3, 1250, 650, 0, 3), (4, 6, 3, 7, 10, 4, 400, 1900, 0, 5)],
    segs=[(3, 7, 1, 0), (7, 11, 1, 1), (15, 19, 3, 0), (19, 20, 4, 0), (20, 24, 5, 0), (24, 28, 5, 1), (28, 29, 5, 2)],
    max=(10, 4, 1250), sizes=(32, 32))

GEO_CASES = [
    GEO_RECORDED,
    # minimizer counts of exactly segl and segl + 1, one and two segments
    ([0, 5, 9], [0, 4, 9], 0, 2, 9, 100, 4, 1 << 30),
    # a query without hits between two with hits, in one chunk
    ([0, 300, 300, 500], [0, 2, 7, 9], 0, 3, 8, 100, 4, 1 << 30),
    # q_stop before the last query, a chunk cut exactly at seed_chunk
    ([0, 400, 1000, 1001, 1500], [0, 1, 2, 3, 4], 0, 3, 40, 100, 4, 1000),
    # a big chunk after a small one
    ([0, 10, 10 + 513 * 10], [0, 1, 3], 0, 2, 4097, 10, 1, 100),
]


def test_seed_geometry(shim):
    for a in GEO_CASES:
        g = geometry(shim, *a)
        assert g == geometry_model(*a)
        for q_lo, q_hi, g_lo, g_hi, ne, nb, hits, h0, big, bq_at in g["chunks"]:
            cb = bk = 0
            for i in range(q_lo, q_hi):                     # cb / bk are the running sums; the chunk's nb closes its entries of bq
                mul, nsl, nseg, seg0, qcb, qbk = g["qg"][i]
                assert (qcb, qbk) == (cb, bk) and g["bq"][bq_at + i - q_lo] == bk
                assert g["has"][i] == int(a[0][i + 1] > a[0][i])
                cb, bk = cb + nsl * nseg, bk + nsl
            assert (ne, nb) == (cb, bk) and g["bq"][bq_at + q_hi - q_lo] == nb
            assert big == int(any(g["qg"][i][1] > SL_SMALL for i in range(q_lo, q_hi)))
            assert hits <= max(a[7], max(y - x for x, y in zip(a[0], a[0][1:])))
        assert all(t == (0,) * 6 for t in g["qg"][:a[2]] + g["qg"][a[3]:])   # the entries outside the group are zero
    assert geometry(shim, *GEO_RECORDED) == GEO_RECORDED_WANT
    g = geometry(shim, *GEO_CASES[1])
    assert [t[2] for t in g["qg"]] == [1, 2] and g["segs"] == [(0, 4, 0, 0), (4, 8, 1, 0), (8, 9, 1, 1)]
    g = geometry(shim, *GEO_CASES[2])
    assert g["has"] == [1, 0, 1] and g["bq"] == [0, 3, 3, 5] and [t[3] for t in g["qg"]] == [0, 1, 1]
    g = geometry(shim, *GEO_CASES[3])
    assert [(c[0], c[1], c[6]) for c in g["chunks"]] == [(0, 2, 1000), (2, 3, 1)]
    g = geometry(shim, *GEO_CASES[4])
    assert [c[8] for c in g["chunks"]] == [0, 1]


GEO_ERRORS = [   # sizes that are only offsets: nothing of their length is allocated
    # one query with 0xfffffff0 hits
    (([0, 0xfffffff0], [0, 1], 0, 1, 10, 7600, 256, 1 << 30), "more than 2^32 seed hits of one query against one index part"),
    # 2^21 segments of one minimizer times 2048 slices: 2^32 pieces in one chunk
    (([0, SL_BIG], [0, 1 << 21], 0, 1, 2 * SL_BIG, 1, 1, 1 << 30), "seed filter: too many (query, slice, segment) pieces in one chunk"),
    # 2^31 segments of one minimizer, one slice: the pieces fit, the segments do not
    (([0, 1], [0, 1 << 31], 0, 1, 10, 7600, 1, 1 << 30), "seed filter: too many segments"),
]


def test_seed_geometry_refuses(shim):
    for a, text in GEO_ERRORS:
        with pytest.raises(ShimError) as e:
            geometry(shim, *a, with_segs=0)
        assert str(e.value) == text
    # just below the second: 2^21 - 1 segments, accepted (the segments are counted, not copied out)
    g = geometry(shim, [0, SL_BIG], [0, (1 << 21) - 1], 0, 1, 2 * SL_BIG, 1, 1, 1 << 30, with_segs=0)
    assert g["max"] == (SL_BIG * ((1 << 21) - 1), SL_BIG, SL_BIG)


# ---- the records' bits ----------------------------------------------------------------------------------------------------------
BITS_FOR = [(0, 1), (1, 1), (2, 2), (2 ** 31 - 1, 31), (2 ** 31, 32)]
# max_nm, max_tlen, max_qlen, n_targets, n_min, max_hits -> jb, db, rb, the filter can run
RECORD_BITS = [
    ((2 ** 31, 2 ** 31 - 1 - 257 - 1000, 1000, 2, 3, 10), (31, 31, 1, 1)),      # exactly 64 bits
    ((2 ** 31, 2 ** 31 - 1 - 257 - 1000, 1000, 3, 3, 10), (31, 31, 2, 0)),      # 65
    ((2 ** 31 + 1, 1000, 1000, 2, 3, 10), (32, 12, 1, 0)),                      # jb beyond 31
    ((100, 2 ** 31 - 257, 0, 2, 3, 10), (7, 32, 1, 0)),                         # db beyond 31
    ((1, 0, 0, 0, 3, 10), (1, 9, 1, 1)),                                        # no target, one minimizer
    ((100, 5000, 3000, 1000, 3, 0x7fff0000 - 1), (7, 14, 10, 1)),
    ((100, 5000, 3000, 1000, 3, 0x7fff0000), (7, 14, 10, 0)),                   # a query with too many hits
] + [((100, 5000, 3000, 1000, n_min, 10), (7, 14, 10, ok)) for n_min, ok in ((1, 0), (2, 1), (15, 1), (16, 0))]
FILTER_FITS = [((3, 31, 31, 1, 10), 1), ((3, 31, 31, 2, 10), 0), ((3, 30, 31, 2, 10), 1), ((3, 32, 20, 1, 10), 0), ((3, 20, 32, 1, 10), 0)]


def test_seed_record_bits(shim):
    for v, b in BITS_FOR:
        assert shim("bits_for", [v]) == [b] == [max(v.bit_length(), 1)]
    for a, want in RECORD_BITS:
        assert tuple(shim("record_bits", list(a))) == want
        max_nm, tl, ql, nt = a[:4]                           # bits that hold 0 .. v, of the largest value of each field
        assert want[:3] == (max((max_nm - 1).bit_length(), 1), max((tl + ql + 257).bit_length(), 1), max((max(nt, 1) - 1).bit_length(), 1))
    for a, want in FILTER_FITS:
        assert shim("filter_fits", list(a)) == [want]


# ---- the lanes' share of the HBM ----------------------------------------------------------------------------------------------
def budget_model(free, reserve, surv_cap, lanes):
    fr = max(free - reserve, 0)
    fr = max(fr - (surv_cap + surv_cap // 2 if reserve else 0), 0)
    return min(max(int(fr * 0.75 / 104.0 / lanes), 1024), 2 ** 31 - 4096)


BUDGET_CASES = [
    ((200 * 10 ** 9, 8 * 10 ** 9, 10 ** 9, 3), 457932692),    # recorded from the parent
    ((10 ** 9, 2 * 10 ** 9, 0, 3), 1024),                     # free < reserve
    ((10 ** 10, 9 * 10 ** 9, 10 ** 9, 3), 1024),              # what is left is below the survivors' share (1.5e9)
    ((10 ** 10, 0, 10 ** 12, 3), 24038461),                   # no reserve: no survivors' share either
    ((1024 * 104 * 4, 0, 0, 3), 1024),                        # 1024 by the formula: the clamp from below at its edge
    ((100000, 0, 0, 1), 1024),                                # below 1024
    ((2 ** 50, 0, 0, 3), 2 ** 31 - 4096),                     # above 2^31 - 4096
]


def test_lane_anchor_budget(shim):
    for a, want in BUDGET_CASES:
        assert shim("budget", list(a)) == [want] == [budget_model(*a)]
    for v, want in ((0, 1024), (1023, 1024), (1024, 1024), (2 ** 31 - 4096, 2 ** 31 - 4096), (2 ** 31 - 4095, 2 ** 31 - 4096), (2 ** 40, 2 ** 31 - 4096)):
        assert shim("clamp", [v]) == [want]


ARENA_CASES = [   # anchor_budget, nA_total -> bytes; the shim is an emulator build: capped at 64 MiB (the device build's 294110544 for the second: recorded from the parent)
    ((1024, 10), 10 * 104 // 9 * 8 + (16 << 20)), ((457932692, 3000000), 64 << 20), ((1024, 0), 104 // 9 * 8 + (16 << 20)), ((1024, 10 ** 9), 1024 * 104 // 9 * 8 + (16 << 20)),
]
FEW_CASES = [   # bucketed, q_begin, n_written, group_hits
    ((1, 0, 25, 100), 1), ((1, 0, 26, 100), 0), ((0, 0, 0, 100), 0), ((1, 1, 25, 100), 0), ((1, 0, 0, 0), 1),
]


def test_arena_and_few(shim):
    assert 3000000 * 104 // 9 * 8 + (16 << 20) == 294110544
    for a, want in ARENA_CASES:
        assert shim("arena", list(a)) == [want]
    for a, want in FEW_CASES:
        assert shim("few", list(a)) == [want]


# ---- the same cases once more, as a program under the sanitizers ----------------------------------------------------------------
def all_cases():
    out = []
    for lanes in (1, 2, 3):
        for _, sizes, hits, g_begin, budget, _ in CUT_CASES + [("", [1] * (lanes * B + 1), None, 0, B, True)]:
            out.append(("cut", cut_words(offs(sizes), offs(hits) if hits else offs(sizes), g_begin, len(sizes), budget, lanes)))
        out.append(("cut", cut_words(offs([1] * 6), offs([(lanes << 24) // 6 + 1] * 6), 0, 6, B, lanes)))
    out += [("cut", cut_words(CUT_AQF, CUT_AQ, g, 9, b, l)) for l, b, g in CUT_RECORDED]
    out += [("subsets", subsets_words(*c)) for c in SUBSET_CASES]
    for nt in (1, 2, 3, 1023, 1024, 4097, 2 ** 31 - 1):
        out += [("geometry", geometry_words([0, ask * 10], [0, 3], 0, 1, nt, 10, 256, 1 << 30)) for ask in (1, 2, SL_SMALL, SL_SMALL + 1, SL_BIG, SL_BIG + 1)]
    out += [("geometry", geometry_words(*a)) for a in GEO_CASES] + [("geometry", geometry_words(*a, with_segs=0)) for a, _ in GEO_ERRORS]
    out.append(("geometry", geometry_words([0, SL_BIG], [0, (1 << 21) - 1], 0, 1, 2 * SL_BIG, 1, 1, 1 << 30, with_segs=0)))
    out += [("bits_for", [v]) for v, _ in BITS_FOR] + [("record_bits", list(a)) for a, _ in RECORD_BITS] + [("filter_fits", list(a)) for a, _ in FILTER_FITS]
    out += [("budget", list(a)) for a, _ in BUDGET_CASES] + [("arena", list(a)) for a, _ in ARENA_CASES] + [("few", list(a)) for a, _ in FEW_CASES]
    return out


def test_the_shim_as_a_program_under_sanitizers(shim, tmp_path):
    exe = str(tmp_path / "mapplan_shim_san")
    build(exe, "-g", "-DMAPPLAN_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    cases = all_cases()
    text = "".join("%s %s\n" % (name, " ".join(map(str, words))) for name, words in cases)
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, words), line in zip(cases, lines):
        try:
            want = " ".join(map(str, shim(name, words, cap=1 << 16))) + " "
        except ShimError as e:
            want = "! " + str(e)
        assert line == want, name

"""The anchor sort between the seed stage and mm_chain_dp (engine.cpp sort_batch; kernels_sort.hpp, kernels_rsort.hpp,
kernels_walk.hpp, kernels_ckpt.hpp, kernels_psort.hpp) against klib's order of equal keys, at the sort's own stage.  The code
exists to reproduce an unstable sort's arrangement of anchors with equal x (lqmap.c:238, ksort.h:84-134); the tables and chain
records see that arrangement only where it tips a threshold, and LQCOV_DEBUG_SORT passes for every tie order.

The model: lqo_sort_128x -- the oracle's restatement of klib's radix_sort_128x, pinned by the golden anchor orders -- once per
query on that query's emitted (x, y) pairs.  Two ways in:

lqcov_debug_sort_anchors runs sort_batch on anchors from the host under a stated geometry (targets, longest target), which
decides the key bytes the passes step over.  Asserted per query: the array equals the model byte for byte, y and its bit 63
included (queries through klib's passes; queries of distinct x, where only one sorted arrangement exists; queries of at most
64 anchors, where the insertion sort is stable); with `want` (the second pass's pruning, k_rs_children): wherever the model's
x >> 32 is a wanted key the anchor is the model's, everywhere else x >> 32 is at most the model's, x >> 32 never descends
inside a query, a wanted key stands nowhere but where the model has it (so every wanted run is there in full), and queries
outside klib's passes are whole.  Refused with LQCOV_E_ARG: an anchor outside the geometry, q_klib on 64 anchors, n >= 2^31.

Synthetic anchors (batch()): x = strand << 63 | rid << 32 | pos; three quarters of the rids on five hot targets (0, 1, the
middle, the last two: adjacent pairs, and the ones with rid >> 24 == 1 above 2^24 targets), the rest anywhere, half of the
positions in the first 256 bases: sub-arrays of every size class at every level.  y = span << 32 | running number, so any swap
of two equal-x anchors shows.  Queries of 0, 1, 64 (ties), 65 (ties), 65 (distinct), 2200 (distinct: the parallel sort), 700
(ties: whole walks of the middle classes) and two of thousands (ties in groups of 2 to 40, a third to a half of the anchors;
one marked exactly on the repeated x, one on a superset as marking by (hash, strand) gives).  LQCOV_WALK_SHIFT=7 unless the case
says otherwise: class caps 32 / 128 / 512 / 1248, checkpoint units 512 and 64.  Every case asserts from stage_times() that the
kernels it is for ran, and from the model's input that at least 50 equal-x groups lie in sub-arrays longer than 64 at its level
and that such a sub-array has the buckets the path needs (byte 0: more than the 128 a register walker holds).

  geometry (targets, longest)   live levels               cases
  12, 3000                      56 (two), 32, 8, 0        two-bucket passes, small-bucket checkpoints, k_sort_walk_reg<1>, byte 0;
                                                          LQCOV_NO_LEVEL_SKIP; walk shifts 4 and 10; LQCOV_WALK=solo + LQCOV_CKPT=0 +
                                                          LQCOV_SORT_TILE=64; LQCOV_PS_SHIFT=5; emulator thread orders; one x 9000 times
  100, 70000                    + 16 (two digits)         k_sort_walk_reg<2> on the rid byte, the pos >> 16 level
  200, 3000                                               k_sort_walk_solo on a rid byte
  40000, 3000                   + 40                      rid >> 8; k_ck_chain256 with LQCOV_CKPT3=1 and 0; LQCOV_PS_SHIFT=7, LQCOV_PS_KEY64
  400000, 3000                  + 48 (digits <= 6)        the few-bucket top pass over rid; walk shifts 4 and 10
  2^24 + 5, 300                 56 with four buckets      any_walk at shift 56, 225 buckets at rid >> 16
  pruning: 12, 40000, 400000 -- a tenth of the (query, strand, rid) keys, each query's first and last key, two adjacent rids, one
  query with nothing wanted.

lqcov_set_debug bit 1 records what the pipeline hands every sort and what comes back (lqcov_get_sort_batches).  On
seed_filter_dataset (-k 9 -w 4; default, and LQCOV_TIES=klib with -X) and _repeat_rich_dataset(n_targets=12, n_queries=2,
glen=21000): kinds 0 and 2 -- each query's emitted anchors are, in order, the rows of all_hits that -Y (and -X) keep, x and y
as lqmap.c:190-197 with MM_SEED_TANDEM and bits 56-63 of y masked; every anchor whose x occurs twice carries LQ_TIE_MARK; the
sorted anchors are the model of the emitted ones; kind 1 -- the emitted anchors are, as a set, the plan's survivors, the sorted
ones ascend and every group of equal x holds the emitted y values; a default run has a kind-2 sort with at least 20 equal-x
groups; nothing is recorded while bit 1 is off.

Which case notices which slip (each seeded into a copy of the sources outside the repository, emulator build, this module's
emulated tests run against it; the pipeline cases are the seed_filter_dataset ones):
  k_rs_children's rank with `xj < el.x` for j < i            every sort, pruned, refusal and pipeline case (26 of 26)
    (and <= for j > i: the insertion sort reversed)
  k_sort_walk_lds replaced by the stable rank                all but t12_shift10 and t400k_shift10, where no sub-array is short
                                                             enough for that walker (24 of 26)
  two-bucket closed form, X and Y lists swapped              the first case that sorts: destinations become garbage and the
                                                             emulator faults; with Y_t into the hole of X_(m-1-t) instead
                                                             (a permutation still): all 26
  the rem == 0 bucket through a partition pass               one key 9000 times (the only bucket of one x above 8192 anchors)
  the prune test `pw.want[lo] <= b` made `<`                 the three pruned cases
  the dropped bucket's fill key one too high                 the three pruned cases
  k_seed_emit reading a minimizer's occurrences backwards    the two pipeline cases (kinds 0 and 2: emitted != all_hits' order)"""
import ctypes as C
import os

import numpy as np
import pytest

from longqc_amd import api
from tests import oracle_bind
from tests.conftest import ROOT
from tests.helpers import all_hits, read_fastx, seed_filter_dataset, slow_emu

MARK = np.uint64(1 << 63)                                       # LQ_TIE_MARK
RS_MIN = 64                                                     # LQ_RS_MIN (ksort.h:81)
U32 = np.uint64(32)


# ---- the model: klib's radix_sort_128x as the oracle restates it, one query at a time --------------------------------------------
_ORA = []


def klib_sort(xy):
    if not _ORA:
        oracle_bind.ensure_oracle()
        ora = C.CDLL(os.path.join(ROOT, "oracle", "liblqcov_oracle.so"))
        ora.lqo_sort_128x.argtypes = [C.c_void_p, C.c_size_t]
        ora.lqo_sort_128x.restype = None
        _ORA.append(ora)
    a = np.ascontiguousarray(xy, dtype=np.uint64).copy()
    if a.shape[0]:
        _ORA[0].lqo_sort_128x(a.ctypes.data_as(C.c_void_p), a.shape[0])
    return a


def model_of(em, off):
    """the model applied to every query's emitted anchors"""
    out = np.empty_like(em)
    for q in range(off.shape[0] - 1):
        out[off[q]:off[q + 1]] = klib_sort(em[off[q]:off[q + 1]])
    return out


# ---- synthetic anchors -----------------------------------------------------------------------------------------------------------
def hot_rids(n_targets):
    """the few targets that hold most anchors: the first two (adjacent), one in the middle, the last two (adjacent; above 2^24
    targets they are the ones whose rid >> 24 is 1)"""
    return sorted({0, 1, n_targets // 2, n_targets - 2, n_targets - 1})


def draw_x(rng, n, n_targets, max_len):
    """n keys strand << 63 | rid << 32 | pos, skewed: three quarters of the rids on hot_rids, the rest anywhere; half of the
    positions in the first 256 bases, so that sub-arrays of more than 64 anchors reach the levels on the position's bytes"""
    hot = np.array(hot_rids(n_targets), dtype=np.uint64)
    w = np.array([8, 2, 3, 1, 2][:hot.shape[0]], dtype=float)
    rid = np.where(rng.random(n) < 0.75, rng.choice(hot, size=n, p=w / w.sum()), rng.integers(0, n_targets, size=n, dtype=np.uint64))
    pos = np.where(rng.random(n) < 0.5, rng.integers(0, min(max_len, 256), size=n, dtype=np.uint64), rng.integers(0, max_len, size=n, dtype=np.uint64))
    return (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)) | (rid << U32) | pos


def distinct_x(rng, n, n_targets, max_len):
    """n keys drawn without replacement, in random order"""
    x = np.zeros(0, dtype=np.uint64)
    while x.shape[0] < n:
        x = np.unique(np.concatenate([x, draw_x(rng, 2 * n + 16, n_targets, max_len)]))
    return rng.permutation(x)[:n]


def tied_x(rng, n, n_targets, max_len):
    """n keys of which a third to a half are copies of another's, in groups of 2 to 40, in random order"""
    copies = int(rng.integers(n // 3, n // 2 + 1)) if n >= 4 else 0
    sizes = []
    while copies > 0:
        g = int(min(rng.integers(2, 41), copies + 1))
        sizes.append(g); copies -= g - 1
    base = distinct_x(rng, n - sum(s - 1 for s in sizes), n_targets, max_len)
    rep = np.ones(base.shape[0], dtype=np.int64)
    rep[:len(sizes)] = sizes
    return rng.permutation(np.repeat(base, rep))


def mark_exact(x):
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] > 1


NOTHING_WANTED = 7                                              # the query of which the pruned sorts want nothing (the first of the two long ones)


def batch(seed, n_targets, max_len, big=(4600, 3700), medium=700, plain=2200, repeat=0):
    """-> dict(em (n, 2) uint64, off, klib): queries of 0, 1, 64 (ties), 65 (ties, klib's passes), 65 (distinct), `plain`
    (distinct: the parallel sort), `medium` (ties: its two strands are whole walks of the middle size classes) and two of several
    thousand with ties -- the first marked exactly on the anchors whose x repeats, the second on a superset (those and a fifth of
    the rest, as marking by (hash, strand) does).  y = span << 32 | running number, so that any swap of two anchors shows.
    repeat: one x that many times over in the first long query (the byte-0 bucket of one key)."""
    rng = np.random.default_rng(9100 + seed)
    xs, klib, superset = [], [], []
    for n, kind in [(0, "d"), (1, "d"), (64, "t"), (65, "t"), (65, "d"), (plain, "d"), (medium, "t"), (big[0], "t"), (big[1], "T")]:
        x = distinct_x(rng, n, n_targets, max_len) if kind == "d" else tied_x(rng, n, n_targets, max_len)
        if repeat and n == big[0]:
            x[rng.choice(n, size=repeat, replace=False)] = x[0]
        xs.append(x); klib.append(1 if kind != "d" and n > RS_MIN else 0); superset.append(kind == "T")
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.uint64)
    n = int(off[-1])
    em = np.zeros((n, 2), dtype=np.uint64)
    em[:, 0] = np.concatenate(xs)
    em[:, 1] = (rng.integers(1, 29, size=n, dtype=np.uint64) << U32) | np.arange(n, dtype=np.uint64)
    for q, x in enumerate(xs):
        m = mark_exact(x) if x.shape[0] else np.zeros(0, dtype=bool)
        if superset[q]:
            m |= rng.random(x.shape[0]) < 0.2
        em[int(off[q]):int(off[q + 1]), 1] |= np.where(m, MARK, np.uint64(0))
    return dict(em=em, off=off.astype(np.int64), klib=np.array(klib, dtype=np.uint32), n_targets=n_targets, max_len=max_len)


GEOM = {                                                        # name -> (n_targets, max_len)
    "t12": (12, 3000), "t100": (100, 70000), "t200": (200, 3000), "t40k": (40000, 3000), "t400k": (400000, 3000), "t16M": ((1 << 24) + 5, 300),
}
_BATCHES = {}


def batch_of(name, repeat=0):
    """one batch per geometry with its model, made once and never changed"""
    key = (name, repeat)
    if key not in _BATCHES:
        b = batch(sorted(GEOM).index(name) + (100 if repeat else 0), *GEOM[name], repeat=repeat, big=(repeat + 3000, 3700) if repeat else (9000, 3700) if name == "t12" else (4600, 3700))
        b["model"] = model_of(b["em"], b["off"])
        b["em"].setflags(write=False); b["model"].setflags(write=False)
        _BATCHES[key] = b
    return _BATCHES[key]


def tie_groups_in_long_subarrays(b, shift):
    """equal-x groups of the queries that go through klib's passes whose sub-array at the level on `shift` -- the anchors of the
    query that share the bytes of x above it -- is longer than 64: the groups whose order that level's pass decides"""
    total = 0
    for q in np.flatnonzero(b["klib"]):
        x = b["em"][b["off"][q]:b["off"][q + 1], 0]
        above = x >> np.uint64(shift + 8) if shift < 56 else np.zeros_like(x)
        _, sub, sub_n = np.unique(above, return_inverse=True, return_counts=True)
        ux, first, cnt = np.unique(x, return_index=True, return_counts=True)
        total += int(np.sum((cnt > 1) & (sub_n[sub.reshape(-1)[first]] > RS_MIN)))
    return total


def distinct_digits_in_long_subarrays(b, shift):
    """the largest number of buckets a sub-array of more than 64 anchors has at the level on `shift`"""
    best = 0
    for q in np.flatnonzero(b["klib"]):
        x = b["em"][b["off"][q]:b["off"][q + 1], 0]
        above = x >> np.uint64(shift + 8) if shift < 56 else np.zeros_like(x)
        for a in np.unique(above):
            s = x[above == a]
            if s.shape[0] > RS_MIN:
                best = max(best, np.unique((s >> np.uint64(shift)) & np.uint64(0xff)).shape[0])
    return best


# ---- the engine's side -----------------------------------------------------------------------------------------------------------
SORT_ENV = ("LQCOV_WALK_SHIFT", "LQCOV_WALK", "LQCOV_CKPT", "LQCOV_CKPT3", "LQCOV_SORT_TILE", "LQCOV_PS_SHIFT", "LQCOV_PS_KEY64", "LQCOV_NO_LEVEL_SKIP",
            "LQCOV_DEBUG_SORT", "LQCOV_SORT", "LQCOV_TIES", "LQ_EMU_ORDER", "LQ_EMU_ORDER_KERNEL", "LQ_EMU_ORDER_THREADS")


def engine(lib, env, monkeypatch):
    for k in SORT_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LQCOV_WALK_SHIFT", "7")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = api.Params()
    lib.lqcov_params_default(p)
    return api.Engine(p, 0, lib=lib)


def sort_on(lib, b, env, monkeypatch, want=None):
    """-> (A, the names of the stages that ran)"""
    eng = engine(lib, env, monkeypatch)
    try:
        eng.set_profiling(2)
        A = eng.debug_sort_anchors(b["em"], b["off"], b["klib"], b["n_targets"], b["max_len"], want)
        ran = {s["name"] for s in eng.stage_times() if s["launches"] > 0}
    finally:
        eng.close()
    return A, ran


def first_diff(A, M, off):
    d = np.flatnonzero(np.any(A != M, axis=1))
    if not d.shape[0]:
        return "equal"
    i = int(d[0]); q = int(np.searchsorted(off, i, "right") - 1)
    return "%d anchors differ, the first at %d (query %d, place %d of %d): x %016x y %016x, the model has x %016x y %016x" % (
        d.shape[0], i, q, i - off[q], off[q + 1] - off[q], A[i, 0], A[i, 1], M[i, 0], M[i, 1])


def check_whole(b, A):
    """every query's anchors equal the model's byte for byte, y and its bit 63 included"""
    M, off = b["model"], b["off"]
    assert A.shape == M.shape
    for q in range(off.shape[0] - 1):
        a, m = A[off[q]:off[q + 1]], M[off[q]:off[q + 1]]
        assert np.array_equal(a, m), "query %d (%d anchors, klib %d): %s" % (q, m.shape[0], b["klib"][q], first_diff(A, M, off))


# name -> (geometry, environment, stages that must have run, the level the case is for, buckets a sub-array there must reach)
CASES = {
    "two_ckpt_small_reg1":  ("t12", {}, ["k_sort_two", "k_ck_prefix", "k_ck_solve", "k_sort_walk_reg<1>ck", "k_sort_walk_reg<1>", "k_sort_walk_lds<16384>"], 32, 12),
    "byte0_many_buckets":   ("t12", {}, ["k_sort_walk_lds<16384>"], 0, 129),
    "reg2_pos16":           ("t100", {}, ["k_sort_walk_reg<2>"], 16, 2),
    "solo_rid_byte":        ("t200", {}, ["k_sort_walk_solo"], 32, 100),
    "rid8_chain256":        ("t40k", {"LQCOV_CKPT3": "1"}, ["k_ck_chain256", "k_sort_walk_solo_ck"], 40, 100),
    "rid8_chain256_ckpt30": ("t40k", {"LQCOV_CKPT3": "0"}, ["k_ck_chain256", "k_sort_walk_solo_ck", "k_sort_walk_solo"], 40, 100),
    "rid16_few_buckets":    ("t400k", {}, ["k_ck_prefix", "k_ck_solve", "k_sort_walk_reg<1>ck"], 48, 5),
    "byte7_four_buckets":   ("t16M", {}, ["k_ck_chain256", "k_sort_walk_solo_ck"], 56, 4),
    "no_level_skip":        ("t12", {"LQCOV_NO_LEVEL_SKIP": "1"}, ["k_sort_two", "k_sort_walk_reg<1>ck"], 32, 12),
    "t12_shift4":           ("t12", {"LQCOV_WALK_SHIFT": "4"}, ["k_sort_walk_reg<1>", "k_sort_walk_lds<4096>"], 32, 12),
    "t12_shift10":          ("t12", {"LQCOV_WALK_SHIFT": "10"}, ["k_sort_walk_reg<1>ck"], 32, 12),
    "t400k_shift4":         ("t400k", {"LQCOV_WALK_SHIFT": "4"}, ["k_sort_walk_reg<1>"], 48, 5),
    "t400k_shift10":        ("t400k", {"LQCOV_WALK_SHIFT": "10"}, ["k_sort_walk_reg<1>ck"], 48, 5),
    "solo_nockpt_tile64":   ("t12", {"LQCOV_WALK": "solo", "LQCOV_CKPT": "0", "LQCOV_SORT_TILE": "64"}, ["k_sort_walk_solo"], 32, 12),
    "ps_shift5":            ("t12", {"LQCOV_PS_SHIFT": "5"}, ["k_ps_finish<1024>"], 32, 12),
    "ps_shift7":            ("t40k", {"LQCOV_PS_SHIFT": "7"}, ["k_ps_hist", "k_ps_scatter"], 40, 100),
    "ps_key64":             ("t40k", {"LQCOV_PS_KEY64": "1"}, ["k_ps_finish<1024>"], 40, 100),
}
EMU_ONLY = {
    "order_reverse":        ("t12", {"LQ_EMU_ORDER": "reverse"}, ["k_sort_two", "k_sort_walk_reg<1>ck"], 32, 12),
    "order_random5":        ("t12", {"LQ_EMU_ORDER": "random:5"}, ["k_sort_two", "k_sort_walk_reg<1>ck"], 32, 12),
}


def run_case(lib, case, monkeypatch):
    geom, env, stages, shift, buckets = case
    b = batch_of(geom)
    n_groups = tie_groups_in_long_subarrays(b, shift)
    assert n_groups >= 50, "only %d equal-x groups in sub-arrays of more than 64 anchors at the level on shift %d" % (n_groups, shift)
    assert distinct_digits_in_long_subarrays(b, shift) >= buckets
    A, ran = sort_on(lib, b, env, monkeypatch)
    missing = [s for s in stages if s not in ran]
    assert not missing, "the case did not reach %s (ran: %s)" % (missing, sorted(ran))
    check_whole(b, A)


@pytest.mark.parametrize("name", sorted(CASES) + sorted(EMU_ONLY))
def test_emulated_sort_is_klibs(emu_lib, name, monkeypatch):
    run_case(emu_lib, CASES.get(name) or EMU_ONLY[name], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_sort_is_klibs(gpu_lib, name, monkeypatch):
    run_case(gpu_lib, CASES[name], monkeypatch)


# ---- one key 9000 times over: a byte-0 bucket is copied in order whatever its length -------------------------------
def run_repeat(lib, monkeypatch):
    b = batch_of("t12", repeat=9000)
    x = b["em"][:, 0]
    ux, cnt = np.unique(x, return_counts=True)
    assert cnt.max() >= 9000 and tie_groups_in_long_subarrays(b, 0) >= 50
    A, ran = sort_on(lib, b, {}, monkeypatch)
    check_whole(b, A)


def test_emulated_one_key_thousands_of_times(emu_lib, monkeypatch):
    run_repeat(emu_lib, monkeypatch)


@pytest.mark.gpu
def test_gpu_one_key_thousands_of_times(gpu_lib, monkeypatch):
    run_repeat(gpu_lib, monkeypatch)


# ---- the second pass's pruning (k_rs_children) -----------------------------------------------------------------------------------
def wanted_keys(b, seed):
    """a random tenth of the (query, strand, rid) keys that occur, plus: the first and the last key of every query, two adjacent
    rids of one strand of the last query; nothing of query NOTHING_WANTED -> sorted uint64 query << 32 | x >> 32"""
    rng = np.random.default_rng(9300 + seed)
    off = b["off"]
    keys = []
    for q in range(off.shape[0] - 1):
        k = np.unique(b["em"][off[q]:off[q + 1], 0] >> U32)
        if q == NOTHING_WANTED or not k.shape[0]:
            continue
        pick = set(k[rng.random(k.shape[0]) < 0.1].tolist()) | {int(k[0]), int(k[-1])}
        if q == off.shape[0] - 2:
            adj = [int(v) for v in k if int(v) + 1 in set(k.tolist())]
            assert adj, "no two adjacent rids in the last query"
            pick |= {adj[len(adj) // 2], adj[len(adj) // 2] + 1}
        keys += [(q << 32) | v for v in pick]
    return np.array(sorted(keys), dtype=np.uint64)


def run_prune(lib, geom, monkeypatch):
    b = batch_of(geom)
    want = wanted_keys(b, sorted(GEOM).index(geom))
    A, ran = sort_on(lib, b, {}, monkeypatch, want=want)
    M, off = b["model"], b["off"]
    n_runs = 0
    for q in range(off.shape[0] - 1):
        a, m = A[off[q]:off[q + 1]], M[off[q]:off[q + 1]]
        wq = (want[(want >> U32) == np.uint64(q)] & np.uint64(0xffffffff))
        ak, mk = a[:, 0] >> U32, m[:, 0] >> U32
        at = np.isin(mk, wq)
        assert np.array_equal(a[at], m[at]), "query %d: a wanted run differs from the model: %s" % (q, first_diff(np.where(at[:, None], a, m), m, np.array([0, m.shape[0]])))
        assert np.all(ak[~at] <= mk[~at]), "query %d: outside the wanted runs a key lies above the model's" % q
        assert np.all(ak[1:] >= ak[:-1]), "query %d: x >> 32 descends" % q
        assert np.array_equal(np.isin(ak, wq), at), "query %d: a wanted key stands where the model has none" % q
        if not b["klib"][q]:
            assert np.array_equal(a, m)                         # (only klib's passes prune)
        n_runs += np.unique(mk[at]).shape[0]
        if q == NOTHING_WANTED:
            assert not at.any()
    assert n_runs == want.shape[0]                              # every wanted key occurs: every wanted run is there in full
    # the pruning did bite: some anchor of a query that went through klib's passes is not the model's
    assert np.any(A != M), "nothing was pruned"


@pytest.mark.parametrize("geom", ["t12", "t40k", "t400k"])
def test_emulated_pruned_sort_keeps_the_wanted_runs(emu_lib, geom, monkeypatch):
    run_prune(emu_lib, geom, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["t12", "t40k", "t400k"])
def test_gpu_pruned_sort_keeps_the_wanted_runs(gpu_lib, geom, monkeypatch):
    run_prune(gpu_lib, geom, monkeypatch)


# ---- what the hook refuses -------------------------------------------------------------------------------------------------------
def run_refusals(lib, monkeypatch):
    b = batch_of("t12")
    eng = engine(lib, {}, monkeypatch)
    try:
        top_rid, top_pos = int(np.max((b["em"][:, 0] >> U32) & np.uint64(0x7fffffff))), int(np.max(b["em"][:, 0] & np.uint64(0xffffffff)))
        for kw in [dict(n_targets=top_rid), dict(max_len=top_pos)]:     # one anchor outside the stated geometry
            g = dict(n_targets=b["n_targets"], max_len=b["max_len"]); g.update(kw)
            with pytest.raises(api.LqcovError):
                eng.debug_sort_anchors(b["em"], b["off"], b["klib"], g["n_targets"], g["max_len"])
        kl = b["klib"].copy(); kl[2] = 1                        # a query of 64 anchors
        with pytest.raises(api.LqcovError):
            eng.debug_sort_anchors(b["em"], b["off"], kl, b["n_targets"], b["max_len"])
        rc = lib.lqcov_debug_sort_anchors(eng.h, b["em"].ctypes.data, 1 << 31, b["off"].astype(np.uint64).ctypes.data, b["klib"].ctypes.data, b["klib"].shape[0], 12, 3000, None, 0)
        assert rc == -1                                          # LQCOV_E_ARG, before anything is read
        A = eng.debug_sort_anchors(b["em"], b["off"], b["klib"], b["n_targets"], b["max_len"])   # ... and the handle still works
        check_whole(b, A)
    finally:
        eng.close()


def test_emulated_hook_refuses_what_it_cannot_sort(emu_lib, monkeypatch):
    run_refusals(emu_lib, monkeypatch)


@pytest.mark.gpu
def test_gpu_hook_refuses_what_it_cannot_sort(gpu_lib, monkeypatch):
    run_refusals(gpu_lib, monkeypatch)


# ---- what the pipeline hands to the sort, and what comes back (lqcov_set_debug bit 1) --------------------------------------------
Y_FLAGS = np.uint64((1 << 56) - 1)                               # (bits 56-63 of y: the engine's own marks)
TANDEM = np.uint64(1 << 42)                                     # MM_SEED_TANDEM (mmpriv.h:18)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> ((target names, target reads, query names, query reads), parameters)"""
    from tests.test_emu_pipeline import _repeat_rich_dataset
    d = tmp_path_factory.mktemp("anchorsort")
    tf, qf = _repeat_rich_dataset(d, 0, n_targets=12, n_queries=2, glen=21000)
    tn, ts, _ = read_fastx(tf)
    qn, qs, _ = read_fastx(qf)
    return {"rr": ((tn, ts, qn, qs), dict(k=12, w=5, min_cnt=3, min_chain_score=40, bw=500)),
            "mix": (seed_filter_dataset(d), dict(k=9, w=4, min_cnt=3, min_chain_score=20, bw=64))}


def expected_anchors(H, rows, qxy, qoff, tandem):
    """the hits `rows` of all_hits as anchors: x = strand << 63 | rid << 32 | target position, y = span << 32 | query coordinate,
    MM_SEED_TANDEM where a neighbour in the query's minimizer list has the same hash (lqmap.c:175-199)"""
    j = H["jl"][rows] + qoff[H["q"][rows]]
    x = (H["rs"][rows].astype(np.uint64) << np.uint64(63)) | (H["rid"][rows].astype(np.uint64) << U32) | H["r"][rows].astype(np.uint64)
    y = ((qxy[j, 0] & np.uint64(0xff)) << U32) | H["y"][rows].astype(np.uint64) | np.where(tandem[j], TANDEM, np.uint64(0))
    return np.stack([x, y], axis=1)


def tandem_of(qxy, qoff):
    key = qxy[:, 0] >> np.uint64(8)
    eq = key[1:] == key[:-1]
    t = np.zeros(key.shape[0], dtype=bool)
    inside = np.ones(key.shape[0] - 1, dtype=bool)
    inside[qoff[1:-1][(qoff[1:-1] > 0) & (qoff[1:-1] < key.shape[0])] - 1] = False      # (neighbours across two queries do not count)
    t[1:] |= eq & inside; t[:-1] |= eq & inside
    return t


def record(lib, data, par, env, monkeypatch, ava=0, off_first=False):
    """one part mapped with recording on -> (the recorded sorts, all_hits, minimizers, query order, the plan's survivors);
    off_first: the part is mapped once before that with recording off, and nothing may have been kept"""
    tn, ts, qn, qs = data
    eng = engine(lib, env, monkeypatch)
    eng.close()
    p = api.Params()
    lib.lqcov_params_default(p)
    p.k, p.w, p.no_self, p.ava = par["k"], par["w"], 1, ava
    p.min_cnt, p.min_chain_score, p.bw = par["min_cnt"], par["min_chain_score"], par["bw"]
    p.min_ovlp = 0; p.min_score_med = p.min_score_good = 160
    eng = api.Engine(p, 0, lib=lib)
    try:
        eng.set_queries(qn, qs)
        pt = eng.part_begin()
        eng.part_add_targets(pt, tn, ts)
        eng.part_build(pt)
        qxy, qoff = eng.query_minimizers()
        txy, _ = eng.part_minimizers(pt, len(tn))
        mid = eng.mid_occ
        perm = eng.query_order().astype(np.int64)
        S = eng.part_seed_survivors(pt) if "LQCOV_TIES" not in env else None
        if off_first:
            eng.part_map(pt); eng.sync()
            eng.set_debug(2)
            assert eng.sort_batches() == [], "sorts were recorded although bit 1 was off"
        eng.set_debug(2)
        eng.part_map(pt); eng.sync()                            # (after off_first a second mapping of the part: the counters add up, the sorts are the same)
        rec = eng.sort_batches()
    finally:
        eng.close()
    qoff = qoff.astype(np.int64)
    H = all_hits(qxy, qoff, txy, [int(s.shape[0]) for s in qs], qn, tn, mid)
    return rec, H, qxy.astype(np.uint64), qoff, perm, S


def check_pipeline(lib, data, par, env, monkeypatch, ava=0, want_kinds=(1, 2), off_first=False):
    rec, H, qxy, qoff, perm, S = record(lib, data, par, env, monkeypatch, ava, off_first)
    qlen = np.array([int(s.shape[0]) for s in data[3]], dtype=np.int64)
    tandem = tandem_of(qxy, qoff)
    keep = ~(H["drop_self"] | H["drop_ava"]) if ava else ~H["drop_self"]
    kinds = [b["kind"] for b in rec]
    assert set(kinds) == set(want_kinds), kinds
    groups_in_kind2 = 0
    for b in rec:
        off = b["off"].astype(np.int64)
        assert off[0] == 0 and off[-1] == b["emitted"].shape[0] == b["sorted"].shape[0] and b["q"].shape[0] == off.shape[0] - 1
        for i, qe in enumerate(b["q"].tolist()):
            qc = int(perm[qe])
            em, so = b["emitted"][off[i]:off[i + 1]], b["sorted"][off[i]:off[i + 1]]
            assert np.all(so[1:, 0] >= so[:-1, 0]), "kind %d, query %s: not ascending" % (b["kind"], data[2][qc])
            if b["kind"] in (0, 2):
                want = expected_anchors(H, np.flatnonzero((H["q"] == qc) & keep), qxy, qoff, tandem)
                got = em.copy(); got[:, 1] &= Y_FLAGS
                assert got.shape == want.shape and np.array_equal(got, want), "kind %d, query %s: the emitted anchors are not the reference's, %s" % (
                    b["kind"], data[2][qc], first_diff(got, want, np.array([0, want.shape[0]])) if got.shape == want.shape else "%d / %d" % (got.shape[0], want.shape[0]))
                rep = mark_exact(em[:, 0]) if em.shape[0] else np.zeros(0, dtype=bool)
                assert np.all((em[rep, 1] & MARK) != 0), "kind %d, query %s: an anchor whose x repeats carries no tie mark" % (b["kind"], data[2][qc])
                assert np.array_equal(so, klib_sort(em)), "kind %d, query %s: %s" % (b["kind"], data[2][qc], first_diff(so, klib_sort(em), np.array([0, em.shape[0]])))
                if b["kind"] == 2:
                    groups_in_kind2 += int(np.sum(np.unique(em[:, 0], return_counts=True)[1] > 1))
            else:
                rows = S["rows"][S["rows"][:, 0] == qe].astype(np.int64)
                j = rows[:, 4] + qoff[qc]
                span = (qxy[j, 0] & np.uint64(0xff)).astype(np.int64)
                qpos = ((qxy[j, 1] & np.uint64(0xffffffff)) >> np.uint64(1)).astype(np.int64)
                ypos = np.where(rows[:, 2] == 1, qlen[qc] - (qpos + 1 - span) - 1, qpos)
                rpos = rows[:, 3] + ypos - qlen[qc] - 256
                want = np.stack([(rows[:, 2].astype(np.uint64) << np.uint64(63)) | (rows[:, 1].astype(np.uint64) << U32) | rpos.astype(np.uint64),
                                 (span.astype(np.uint64) << U32) | ypos.astype(np.uint64) | np.where(tandem[j], TANDEM, np.uint64(0))], axis=1)
                got = em.copy(); got[:, 1] &= Y_FLAGS
                by = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]
                assert got.shape == want.shape and np.array_equal(by(got), by(want)), "first pass, query %s: the emitted anchors are not the plan's survivors" % data[2][qc]
                assert np.array_equal(by(so), by(em)), "first pass, query %s: a group of equal x does not hold the emitted y values" % data[2][qc]
    if 2 in want_kinds:
        assert groups_in_kind2 >= 20, "%d equal-x groups in the second pass's sorts" % groups_in_kind2
    return rec


PIPE = [("rr", {}, 0, (1, 2)), ("rr", {"LQCOV_TIES": "klib"}, 0, (0,)), ("mix", {}, 0, (1, 2)), ("mix", {"LQCOV_TIES": "klib"}, 1, (0,))]
PIPE_IDS = ["rr", "rr_ties_klib", "mix", "mix_ties_klib_X"]
# (the repeat-rich set takes two minutes a mapping on the emulator: its emulated forms run with LQCOV_SLOW_TESTS=1, as the other
# long emulator runs of the suite do; the smaller set stays in the default run and both have their GPU forms)
PIPE_EMU = [pytest.param(*c, id=i, marks=slow_emu if c[0] == "rr" else ()) for c, i in zip(PIPE, PIPE_IDS)]


@pytest.mark.parametrize("name,env,ava,kinds", PIPE_EMU)
def test_emulated_pipeline_hands_the_sort_the_references_anchors(emu_lib, inputs, name, env, ava, kinds, monkeypatch):
    check_pipeline(emu_lib, inputs[name][0], inputs[name][1], env, monkeypatch, ava, kinds, off_first=name == "mix" and not env)


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,ava,kinds", PIPE, ids=PIPE_IDS)
def test_gpu_pipeline_hands_the_sort_the_references_anchors(gpu_lib, inputs, name, env, ava, kinds, monkeypatch):
    check_pipeline(gpu_lib, inputs[name][0], inputs[name][1], env, monkeypatch, ava, kinds, off_first=name == "mix" and not env)

"""The seed filter's survivor set (kernels_seed.hpp: k_seed_count, k_seed_scatter, k_seed_decide, k_seed_decide_big,
k_seed_collect) against a plain numpy model, at the filter's own stage.  The header promises that no hit that could reach a
chain is dropped, and that a hit survives iff its (query, target, strand) pair holds n_min hits and the gap-free stretch of
non-empty diagonal bins around its own bin holds n_min hits.  The rest of the suite sees the filter through the final table
and `last_written < emitted` only: a filter that keeps too much gives the same table, and one that drops a hit of a real
component changes a row only where that tips one of the row's thresholds.

S is what lqcov_part_seed_survivors returns for a part built with the queries set (the plan is made by lqcov_part_build; no
mapping is involved).  The model takes the minimizer lists (Engine.query_minimizers / part_minimizers), Engine.mid_occ, the
read lengths and the names from the engine, nothing else:
  All  every occurrence in the part of every query minimizer whose list is shorter than mid_occ (lqmap.c:166-173), with the
       query coordinate of lqmap.c:190-197 and diagonal = target position - query coordinate + query length + 256
  P    the hits whose (query, target, relative strand) pair holds n_min = max(-n, ceil(-m / k)) hits
  M    the hits of P for which the window rule holds, written from sd_window_alive's comment on bins diagonal >> dshift (dshift:
       the smallest s >= 1 with 2^s > bw), with plain counts; a pair whose diagonals can take more than 8192 bins is kept whole
  L    from first principles (chain.c:47-56): inside a pair two hits interact when 0 < dq <= max_gap, 0 < dr <= max_gap and
       |dr - dq| <= bw; the hits whose connected component holds n_min hits
The self diagonal of -Y and, with -X, the targets named below the query (lqmap.c:180-187) leave P, M and L after the counting,
as in the kernels.  Asserted: L <= M <= P <= All (model alone); S == M for the default geometry and for those that only
repartition the work; M <= S <= All (LQCOV_SEED_PAIR_BITS=3, LQCOV_SEED_HWORDS=40) or <= P (LQCOV_SEED_BIGCAP below a bucket:
pairs only) where counters alias or run out; L <= S and no row twice in every case; the offsets ascend, every query's rows lie
between its offsets and carry its number, last_written after part_map is the row count; two engines give the same bytes
(emulator: also with the threads in reverse and in random order); n_min 16 and 1 and LQCOV_FILTER=0 are reported as not bucketed;
with LQCOV_SEED_SURV_MAX small the plan stops at a group of queries and is exact for those.  The getter itself: a buffer too small gets
the needed size and nothing beyond its end; a part without a plan is an error.

Inputs (tests.helpers.seed_filter_dataset, -k 9 -w 4): limits_dataset's targets and its seven queries of 1.9-2.9 kb (overlaps on
both strands, tandem repeats: 1800-14000 surviving hits a query), 30 unrelated random targets of 1.5-3.5 kb (several chance
hits to a pair, spread over its diagonals: what the window drops), 120 of 300-900 bases (a third of their pairs hold one hit:
what the pair rule drops), and two queries once more as targets under their own names (2216 hits on the self diagonal; -X
drops 6885).  65 678 hits, mid_occ 53; over n_min 2, 3, 4 (where the
window is exact), 5, 9, 15 (where it is generous) x bw 500, 64, 8, 100, and five of these with -X, the pair rule drops 529-6460
hits, the window 351-6247, 51 846-62 104 survive, and M - L holds 16-1763 hits (test_model_is_nested_and_the_inputs_have_teeth
asserts at least 100 hits, of at least two queries, in each class of each case).  The same test asserts that the histograms of
all pairs of one query fit one bucket's LQ_SD_HWORDS in every case -- pairs that find no room are kept whole by design
(sd_rank_pairs), and S == M is owed only where that cannot happen, whatever the buckets are.  seed_filter_long_pair: a query and
a target of 9 kb at bw 0 (bins of two, 9110 of them: kept whole, where the window would drop 209 of its hits) among eight
targets of 1.2 kb whose pairs are windowed.

Which case notices which slip (each seeded into a copy of the sources, emulator build, the whole module run against it):
  `tot >= n_min` -> `>` in sd_window_alive           every case that compares survivors (all but determinism and not-bucketed)
  sd_window_alive always true                         every exact case (the M <= S <= All cases pass, as they must)
  `c[i] >= dp.n_min` -> `>` in sd_rank_pairs          every exact case but nmin4/5/9_bw8 and nmin3_bw8_X; LQCOV_SEED_HWORDS=40 and
                                                      BIGCAP (a hit of M missing)
  the same threshold one too low (`c[i] + 1 >=`)      n_min 5, 9, 15 at bw 500, 9 and 15 at bw 64 and 100 (where the window is
                                                      exact it drops what the pair rule let through: n_min 2-4 cannot see it)
  reach from one bin too near, n_min 3 (r1 | l1)      every n_min 3 case, the long pair, the groups, last_written
  reach from one bin too near, n_min >= 4 (r2 | l2)   every case of n_min 4, 5, 9, 15
  (reach from one bin too far changes nothing: for n_min <= 4 a stretch that reaches the edge holds n_min hits anyway)
  dp.dshift one smaller / one larger                  every exact case but the long pair, and three of the four aliasing cases (a hit
                                                      of M missing) / every exact case, the long pair included
  sd_hist_words one word short, (nb + 13) >> 3        none, and none can: the places dbin .. dbin + 6 that a window reads end at
                                                      nb + 5, inside word (nb + 5) >> 3, the last of (nb + 13) >> 3; the kernel's
                                                      (nb + 21) >> 3 keeps one word to spare (two words short: see below)
  the self-diagonal drop skipped                      every case that compares survivors but the long pair (which has no same name)
  one record lost per tile of k_seed_scatter          every case (a stale record takes its place; the emulator then faults)
  k_seed_collect copying n - 1 rows                   every case that compares survivors
  sd_hist_words two words short, (nb + 5) >> 3        every bw 500 case of test_emulated_survivors_are_the_models (the top bins of
                                                      a pair of 12-14 bins land in the next pair's words)"""
import numpy as np
import pytest

from longqc_amd import api
from tests.helpers import all_hits, seed_filter_dataset, seed_filter_long_pair

K, W = 9, 4
MAX_GAP = 10000
HBINS_MAX = 8192                                                # LQ_SD_HBINS_MAX
HWORDS = 12288                                                  # LQ_SD_HWORDS


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """name -> (target names, target reads, query names, query reads)"""
    return {"mix": seed_filter_dataset(tmp_path_factory.mktemp("seedfilter")), "long": seed_filter_long_pair()}


# ---- the model -----------------------------------------------------------------------------------------------------------------
def n_min_of(min_cnt, min_score, k=K):
    """hits a chain needs: it takes min_cnt anchors and scores at most k an anchor (run_n_min, engine.hpp, without -H)"""
    return max(min_cnt, 1, -(-min_score // k))


def dshift_of(bw):
    s = 1
    while (1 << s) <= max(bw, 0):
        s += 1
    return s


def _group(*cols):
    """-> (group number of every row, rows per group) for the rows grouped by the columns"""
    key = np.stack(cols, axis=1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return inv.reshape(-1), cnt


def pair_rule(H, n_min):
    """P: the hits whose (query, target, relative strand) holds n_min hits"""
    pair, cnt = _group(H["q"], H["rid"], H["rs"])
    return cnt[pair] >= n_min, pair


def window_rule(H, pair, inP, n_min, bw, qlen, tlen, whole_rule=True):
    """M: the hits of P whose own diagonal bin, or the gap-free stretch of non-empty bins around it, holds n_min hits -- as far as
    the kernel's window of seven bins sees (sd_window_alive's comment): the own bin and min(n_min - 1, 3) bins on either side; a
    stretch of non-empty bins that reaches the window's edge is taken as long enough, one that ends inside is counted.  Bins
    are diagonal >> dshift with plain counts, per pair, of the hits of pairs in P.  A pair whose diagonals can take more than
    LQ_SD_HBINS_MAX bins is kept whole (sd_rank_pairs)."""
    ds = dshift_of(bw)
    side = min(n_min - 1, 3)
    b = H["diag"] >> ds
    assert b.max() + 8 < (1 << 30)
    key = pair * (1 << 30) + b + 4
    uk, cnt = np.unique(key[inP], return_counts=True)

    def count_at(k):
        i = np.searchsorted(uk, k)
        i = np.minimum(i, uk.shape[0] - 1)
        return np.where(uk[i] == k, cnt[i], 0)

    tot = count_at(key)
    alive = np.zeros(key.shape[0], dtype=bool)
    for sgn in (1, -1):
        open_ = np.ones(key.shape[0], dtype=bool)                # the stretch has reached this far without a gap
        for dist in range(1, side + 1):
            c = count_at(key + sgn * dist)
            open_ &= c > 0
            tot = tot + np.where(open_, c, 0)
        alive |= open_                                           # (the bin at the window's edge is part of the stretch)
    alive |= tot >= n_min
    if whole_rule:
        nb = ((np.asarray(qlen, dtype=np.int64)[H["q"]] + np.asarray(tlen, dtype=np.int64)[H["rid"]] + 256) >> ds) + 1
        alive |= nb > HBINS_MAX
    return alive & inP


def component_sizes(H, pair, bw, max_gap=MAX_GAP):
    """Inside a pair two hits interact when 0 < dq <= max_gap, 0 < dr <= max_gap and |dr - dq| <= bw (chain.c:47-56) -> the size
    of every hit's connected component.  L = the hits whose component holds n_min hits (such a hit's pair holds them too)."""
    size = np.ones(pair.shape[0], dtype=np.int64)
    idx = np.argsort(pair, kind="stable")
    cuts = np.flatnonzero(np.diff(pair[idx])) + 1
    for g in np.split(idx, cuts):
        n = g.shape[0]
        if n < 2:
            continue
        y, r = H["y"][g], H["r"][g]
        dq, dr = y[:, None] - y[None, :], r[:, None] - r[None, :]
        A = (dq > 0) & (dq <= max_gap) & (dr > 0) & (dr <= max_gap) & (np.abs(dr - dq) <= bw)
        A |= A.T
        np.fill_diagonal(A, True)
        lab = np.arange(n, dtype=np.int32)
        while True:                                              # the smallest label in reach, then pointer jumping
            new = np.where(A, lab[None, :], np.int32(n)).min(axis=1)
            new = new[new]
            if np.array_equal(new, lab):
                break
            lab = new
        size[g] = np.bincount(lab, minlength=n)[lab]
    return size


def rows_of(H, mask):
    """the hits of `mask` as sorted rows (query, rid, relative strand, diagonal, minimizer index inside the query)"""
    m = np.stack([H[c][mask] for c in ("q", "rid", "rs", "diag", "jl")], axis=1)
    return m[np.lexsort(m.T[::-1])]


_MODELS = {}


def model(mini, names, n_min, bw, ava):
    """-> (H, masks): All as columns, and P, M, L with the hits that -Y (and -X) drop taken out after counting, as the kernels do;
    Praw: P before that.  One table of hits per input, one set of components per band."""
    qxy, qoff, txy, toff, mid = mini
    tn, ts, qn, qs = names
    qlen, tlen = [int(s.shape[0]) for s in qs], [int(s.shape[0]) for s in ts]
    hk = (hash(qxy.tobytes()), hash(txy.tobytes()), mid)
    if hk not in _MODELS:
        H = all_hits(qxy, qoff, txy, qlen, qn, tn, mid)
        _MODELS[hk] = (H, _group(H["q"], H["rid"], H["rs"])[0], {}, {})
    H, pair, comp, memo = _MODELS[hk]
    if (n_min, bw, ava) not in memo:
        if bw not in comp:
            comp[bw] = component_sizes(H, pair, bw)
        inP, _ = pair_rule(H, n_min)
        M = window_rule(H, pair, inP, n_min, bw, qlen, tlen)
        keep = ~(H["drop_self"] | H["drop_ava"]) if ava else ~H["drop_self"]
        memo[(n_min, bw, ava)] = dict(pair=pair, Praw=inP, drop=~keep, P=inP & keep, M=M & keep, L=(comp[bw] >= n_min) & keep,
                                      M_windowed=window_rule(H, pair, inP, n_min, bw, qlen, tlen, whole_rule=False) & keep)
    return H, memo[(n_min, bw, ava)]


# ---- the engine's side ---------------------------------------------------------------------------------------------------------
def plan(lib, names, par, env, monkeypatch, then_map=False):
    """One part built with the queries set (the plan is made by part_build) -> (minimizers and mid_occ for the model, the getter's
    answer with the queries numbered as the caller numbers them, last_written after part_map if asked for)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tn, ts, qn, qs = names
    p = api.Params()
    lib.lqcov_params_default(p)
    p.k, p.w, p.no_self, p.ava = K, W, 1, int(par.get("ava", 0))
    p.min_cnt, p.min_chain_score, p.bw, p.max_gap = par["min_cnt"], par["min_chain_score"], par["bw"], MAX_GAP
    p.min_ovlp = 0; p.min_score_med = p.min_score_good = 160
    eng = api.Engine(p, 0, lib=lib)
    try:
        eng.set_queries(qn, qs)
        pt = eng.part_begin()
        eng.part_add_targets(pt, tn, ts)
        eng.part_build(pt)
        qxy, qoff = eng.query_minimizers()
        txy, toff = eng.part_minimizers(pt, len(tn))
        mini = (qxy, qoff, txy, toff, eng.mid_occ)
        S = eng.part_seed_survivors(pt)
        perm = eng.query_order().astype(np.int64)               # perm[engine index] = the caller's index
        written = None
        if then_map:
            eng.part_map(pt)
            eng.sync()
            written = eng.map_stats()["last_written"]
    finally:
        eng.close()
    assert sorted(perm.tolist()) == list(range(len(qn)))
    S["raw"] = S["rows"].copy()
    S["engine_q"] = S["rows"][:, 0].astype(np.int64)
    S["rows"] = S["rows"].astype(np.int64)
    S["rows"][:, 0] = perm[S["engine_q"]] if S["rows"].shape[0] else 0
    S["perm"] = perm
    return mini, S, written


def check_layout(S, n_q):
    """the offsets ascend from 0, every query's rows lie between its offsets and carry its number"""
    off = S["off"].astype(np.int64)
    assert 0 <= S["q_begin"] <= S["q_end"] <= n_q
    assert off.shape[0] == S["q_end"] - S["q_begin"] + 1 and off[0] == 0 and np.all(np.diff(off) >= 0)
    assert off[-1] == S["rows"].shape[0], "the last offset %d, %d rows" % (off[-1], S["rows"].shape[0])
    assert np.array_equal(S["engine_q"], np.repeat(np.arange(S["q_begin"], S["q_end"]), np.diff(off))), "rows outside their query's offsets"


def _tuples(rows):
    return set(map(tuple, rows.tolist()))


def _first_diff(got, want):
    g, w = _tuples(got), _tuples(want)
    return "%d rows only in the engine's set (first %r), %d only in the model's (first %r)" % (len(g - w), min(g - w, default=None), len(w - g), min(w - g, default=None))


def check_survivors(lib, names, par, env, monkeypatch, exact=True, upper="All", groups=False, then_map=False):
    """S against the model, per query: S == M (exact) or M <= S <= upper; L <= S; no row twice; the layout"""
    mini, S, written = plan(lib, names, par, env, monkeypatch, then_map)
    n_min = n_min_of(par["min_cnt"], par["min_chain_score"])
    n_q = len(names[2])
    assert S["bucketed"] and S["n_min"] == n_min
    check_layout(S, n_q)
    if groups:
        assert 0 < S["q_end"] < n_q, "the plan holds the queries %d..%d of %d: no second group" % (S["q_begin"], S["q_end"], n_q)
    else:
        assert (S["q_begin"], S["q_end"]) == (0, n_q)
    H, R = model(mini, names, n_min, par["bw"], par.get("ava", 0))
    rows = S["rows"]
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0], "a row occurs twice"
    held = S["perm"][S["q_begin"]:S["q_end"]]                   # the caller's numbers of the queries the plan holds
    for qi in sorted(held.tolist()):
        of_q = H["q"] == qi
        got = rows[rows[:, 0] == qi]
        got = got[np.lexsort(got.T[::-1])]
        want = rows_of(H, R["M"] & of_q)
        name = names[2][qi]
        if exact:
            assert got.shape == want.shape and np.array_equal(got, want), "%s: S != M, %s" % (name, _first_diff(got, want))
        else:
            g = _tuples(got)
            assert _tuples(want) <= g, "%s: a hit of M is missing, %s" % (name, _first_diff(got, want))
            up = rows_of(H, (R["P"] if upper == "P" else ~R["drop"]) & of_q)
            assert g <= _tuples(up), "%s: a survivor outside %s, %s" % (name, upper, _first_diff(got, up))
        assert _tuples(rows_of(H, R["L"] & of_q)) <= _tuples(got), "%s: a hit of a component of %d hits was dropped" % (name, n_min)
    if then_map:
        assert written == rows.shape[0], "last_written %d, %d rows in the plan" % (written, rows.shape[0])
    return S


def check_deterministic(lib, names, par, envs, monkeypatch):
    """two engines (one per environment) give byte-identical rows and offsets"""
    first = None
    for env in envs:
        for k in ("LQ_EMU_ORDER",):
            monkeypatch.delenv(k, raising=False)
        _, S, _ = plan(lib, names, par, env, monkeypatch)
        assert S["bucketed"] and S["raw"].shape[0] > 1000
        if first is None:
            first = S
        else:
            assert S["raw"].tobytes() == first["raw"].tobytes() and S["off"].tobytes() == first["off"].tobytes(), env


def check_not_bucketed(lib, names, monkeypatch):
    """a chain of one anchor, a threshold beyond the 4-bit bins, no filter asked for: the getter says that nothing was filtered"""
    for par, env in ((dict(min_cnt=16, min_chain_score=40, bw=64), {}), (dict(min_cnt=1, min_chain_score=9, bw=64), {}),
                     (dict(THRESH[3], bw=64), {"LQCOV_FILTER": "0"})):
        mini, S, _ = plan(lib, names, par, env, monkeypatch)
        assert not S["bucketed"] and S["rows"].shape[0] == 0, par
        assert (S["q_begin"], S["q_end"]) == (0, len(names[2]))
        H, _ = model(mini, names, 3, 64, 0)
        assert np.all(np.diff(S["off"].astype(np.int64)) >= 0) and S["off"][0] == 0
        # (every hit is written: the offsets are those of All without the self diagonal)
        want = np.bincount(H["q"][~H["drop_self"]], minlength=len(names[2]))[S["perm"]]
        assert np.array_equal(np.diff(S["off"].astype(np.int64)), want), par


def check_getter_contract(lib, names, monkeypatch):
    """a buffer too small: the needed size comes back and nothing is written beyond the buffer; no plan (part not built, or built
    before any queries were set): an error, not an empty answer"""
    import ctypes as C
    tn, ts, qn, qs = names
    p = api.Params()
    lib.lqcov_params_default(p)
    p.k, p.w, p.no_self, p.bw = K, W, 1, BASE["bw"]
    p.min_cnt, p.min_chain_score = BASE["min_cnt"], BASE["min_chain_score"]
    monkeypatch.setenv("LQCOV_PLAN_AHEAD", "0")
    eng = api.Engine(p, 0, lib=lib)
    try:
        eng.set_queries(qn, qs)
        pt = eng.part_begin()
        eng.part_add_targets(pt, tn[:40], ts[:40])
        eng.part_build(pt)
        with pytest.raises(api.LqcovError):
            eng.part_seed_survivors(pt)
    finally:
        eng.close()
    monkeypatch.delenv("LQCOV_PLAN_AHEAD")
    eng = api.Engine(p, 0, lib=lib)
    try:
        eng.set_queries(qn, qs)
        pt = eng.part_begin()
        eng.part_add_targets(pt, tn[:40], ts[:40])
        with pytest.raises(api.LqcovError):
            eng.part_seed_survivors(pt)
        eng.part_build(pt)
        full = eng.part_seed_survivors(pt)
        assert full["bucketed"] and full["rows"].shape[0] > 1000 and full["off"].shape[0] == len(qn) + 1
        info = np.zeros(4, dtype=np.uint32)
        off = np.full(len(qn) + 1, 2 ** 64 - 1, dtype=np.uint64)
        rows = np.full((20, 5), 2 ** 32 - 1, dtype=np.uint32)
        n = C.c_uint64()
        assert lib.lqcov_part_seed_survivors(eng.h, pt, info.ctypes.data, off.ctypes.data, 2, rows.ctypes.data, 10, C.byref(n)) == 0
        assert n.value == full["rows"].shape[0] and info.tolist() == [1, full["n_min"], 0, len(qn)]
        assert np.array_equal(rows[:10], full["rows"][:10]) and np.all(rows[10:] == 2 ** 32 - 1)
        assert np.array_equal(off[:2], full["off"][:2]) and np.all(off[2:] == 2 ** 64 - 1)
    finally:
        eng.close()


# ---- the cases -----------------------------------------------------------------------------------------------------------------
THRESH = {2: dict(min_cnt=2, min_chain_score=18), 3: dict(min_cnt=3, min_chain_score=20), 4: dict(min_cnt=3, min_chain_score=33),
          5: dict(min_cnt=5, min_chain_score=40), 9: dict(min_cnt=3, min_chain_score=80), 15: dict(min_cnt=15, min_chain_score=40)}
BANDS = (500, 64, 8, 100)
GRID = [dict(THRESH[n], bw=bw) for bw in BANDS for n in sorted(THRESH)] + \
       [dict(THRESH[n], bw=bw, ava=1) for n, bw in ((2, 64), (3, 500), (3, 8), (4, 100), (15, 64))]
BASE = dict(THRESH[3], bw=64)
# geometries that only repartition the work: many small buckets (more slices; pieces of a few hits), segments of seven minimizers,
# a chunk of queries per query, buckets beyond the block's registers decided in passes over their targets
EXACT_ENVS = [{"LQCOV_SEED_BUCKET": "64"}, {"LQCOV_SEED_BUCKET": "300"}, {"LQCOV_SEED_SEGL": "7"}, {"LQCOV_SEED_CHUNK": "1024"}, {"LQCOV_SEED_DCAP": "300"},
              {"LQCOV_SEED_DCAP": "300", "LQCOV_SEED_BUCKET": "300", "LQCOV_SEED_SEGL": "7"}]
EXACT_CASES = [(BASE, e) for e in EXACT_ENVS] + [(dict(THRESH[2], bw=8), EXACT_ENVS[4]), (dict(THRESH[4], bw=100, ava=1), EXACT_ENVS[5])]
# counters that alias or run out only ever add
LOOSE_CASES = [(BASE, {"LQCOV_SEED_PAIR_BITS": "3"}, "All"), (BASE, {"LQCOV_SEED_HWORDS": "40"}, "All"),
               (dict(THRESH[2], bw=8), {"LQCOV_SEED_PAIR_BITS": "3", "LQCOV_SEED_HWORDS": "40", "LQCOV_SEED_DCAP": "300"}, "All"),
               (BASE, {"LQCOV_SEED_DCAP": "300", "LQCOV_SEED_BIGCAP": "1000"}, "P")]
GROUP_ENV = {"LQCOV_SEED_SURV_MAX": "20000", "LQCOV_SEED_CHUNK": "1024"}
LONG = dict(THRESH[3], bw=0)


def _id(v):
    if isinstance(v, str):
        return v
    if any(k.startswith("LQ") for k in v):
        return "+".join("%s=%s" % (k.replace("LQCOV_SEED_", ""), x) for k, x in sorted(v.items()))
    return "nmin%d_bw%d%s" % (n_min_of(v["min_cnt"], v["min_chain_score"]), v["bw"], "_X" if v.get("ava") else "")


@pytest.fixture(scope="module")
def emu_mini(emu_lib, reads):
    """the minimizers and mid_occ of both inputs, from one build each: all the model takes from an engine"""
    mp = pytest.MonkeyPatch()
    try:
        return {name: plan(emu_lib, reads[name], BASE, {}, mp)[0] for name in reads}
    finally:
        mp.undo()


def _words(H, R, names, bw):
    """-> (the histogram space that the pairs of P of one query take at most, in words of eight bins: sd_hist_words for the bins
    that query + target length + 256 diagonals can take; the pairs beyond LQ_SD_HBINS_MAX bins, which take none)"""
    tn, ts, qn, qs = names
    qlen, tlen = np.array([s.shape[0] for s in qs]), np.array([s.shape[0] for s in ts])
    pr = np.unique(np.stack([H["q"][R["Praw"]], H["rid"][R["Praw"]], H["rs"][R["Praw"]]], axis=1), axis=0)
    nb = ((qlen[pr[:, 0]] + tlen[pr[:, 1]] + 256) >> dshift_of(bw)) + 1
    return np.bincount(pr[:, 0], weights=np.where(nb <= HBINS_MAX, (nb + 21) >> 3, 0)).max(), np.count_nonzero(nb > HBINS_MAX)


def test_model_is_nested_and_the_inputs_have_teeth(emu_mini, reads):
    """From the model alone: L <= M <= P <= All; in every threshold / band case each of All - P (dropped by the pair rule), P - M
    (held by the pair rule, dropped by the window) and M (kept) holds at least 100 hits, of at least two queries; every query's
    histograms fit LQ_SD_HWORDS whatever the buckets are (else pairs are kept whole for want of room and S == M is not owed); M - L
    is not empty over the module; the self diagonal and -X drop hits that would survive; bw 100 and 64 share their bins and
    differ in L; the long pair is kept whole and the window would have dropped some of it."""
    names = reads["mix"]
    tn, ts, qn, qs = names
    conservative = 0
    for par in GRID + [c[0] for c in EXACT_CASES + LOOSE_CASES]:
        n_min, bw, ava = n_min_of(par["min_cnt"], par["min_chain_score"]), par["bw"], par.get("ava", 0)
        H, R = model(emu_mini["mix"], names, n_min, bw, ava)
        assert not np.any(R["L"] & ~R["M"]) and not np.any(R["M"] & ~R["P"]) and not np.any(R["P"] & ~R["Praw"]), _id(par)
        for what, mask in (("All - P", ~R["Praw"]), ("P - M", R["P"] & ~R["M"]), ("M", R["M"])):
            per_q = np.bincount(H["q"][mask], minlength=len(qn))
            assert per_q.sum() >= 100 and np.count_nonzero(per_q) >= 2, (_id(par), what, per_q)
        conservative += int(np.count_nonzero(R["M"] & ~R["L"]))
        assert np.any(R["Praw"] & H["drop_self"]) and (not ava or np.any(R["Praw"] & H["drop_ava"] & ~H["drop_self"])), _id(par)
        assert _words(H, R, names, bw)[0] <= HWORDS and _words(H, R, names, bw)[1] == 0, _id(par)
    assert conservative > 0
    for n in (3, 4):
        a, b = model(emu_mini["mix"], names, n, 64, 0)[1], model(emu_mini["mix"], names, n, 100, 0)[1]
        assert np.array_equal(a["M"], b["M"]) and np.count_nonzero(a["L"] != b["L"]) > 0
    names = reads["long"]
    H, R = model(emu_mini["long"], names, 3, 0, 0)
    assert not np.any(R["L"] & ~R["M"]) and not np.any(R["M"] & ~R["P"])
    assert _words(H, R, names, 0)[0] <= HWORDS and _words(H, R, names, 0)[1] == 2
    long_pair = (H["q"] == 0) & (H["rid"] == 0)
    assert np.count_nonzero(R["M"] & ~R["M_windowed"]) >= 100 and not np.any(R["M"] & ~R["M_windowed"] & ~long_pair)
    assert np.count_nonzero(R["P"] & ~R["M"]) >= 100 and np.any(R["M_windowed"] & ~long_pair)


@pytest.mark.parametrize("par", GRID, ids=_id)
def test_emulated_survivors_are_the_models(emu_lib, reads, monkeypatch, par):
    check_survivors(emu_lib, reads["mix"], par, {}, monkeypatch)


@pytest.mark.parametrize("par,env", EXACT_CASES, ids=_id)
def test_emulated_survivors_whatever_the_partition(emu_lib, reads, monkeypatch, par, env):
    check_survivors(emu_lib, reads["mix"], par, env, monkeypatch)


@pytest.mark.parametrize("par,env,upper", LOOSE_CASES, ids=_id)
def test_emulated_counters_that_alias_only_add(emu_lib, reads, monkeypatch, par, env, upper):
    check_survivors(emu_lib, reads["mix"], par, env, monkeypatch, exact=False, upper=upper)


def test_emulated_long_pair_is_kept_whole(emu_lib, reads, monkeypatch):
    check_survivors(emu_lib, reads["long"], LONG, {}, monkeypatch)


def test_emulated_plan_is_what_the_first_pass_writes(emu_lib, reads, monkeypatch):
    check_survivors(emu_lib, reads["mix"], BASE, {}, monkeypatch, then_map=True)


def test_emulated_groups_of_queries(emu_lib, reads, monkeypatch):
    check_survivors(emu_lib, reads["mix"], BASE, GROUP_ENV, monkeypatch, groups=True)


def test_emulated_survivors_in_one_order_whatever_the_threads_do(emu_lib, reads, monkeypatch):
    check_deterministic(emu_lib, reads["mix"], BASE, [{}, {}, {"LQ_EMU_ORDER": "reverse"}, {"LQ_EMU_ORDER": "random:5"}], monkeypatch)
    check_deterministic(emu_lib, reads["mix"], BASE, [dict(EXACT_ENVS[5]), dict(EXACT_ENVS[5], LQ_EMU_ORDER="reverse"), dict(EXACT_ENVS[5], LQ_EMU_ORDER="random:5")], monkeypatch)


def test_emulated_not_bucketed(emu_lib, reads, monkeypatch):
    check_not_bucketed(emu_lib, reads["mix"], monkeypatch)


def test_emulated_getter_contract(emu_lib, reads, monkeypatch):
    check_getter_contract(emu_lib, reads["mix"], monkeypatch)


@pytest.mark.gpu
def test_gpu_getter_contract(gpu_lib, reads, monkeypatch):
    check_getter_contract(gpu_lib, reads["mix"], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("par", GRID, ids=_id)
def test_gpu_survivors_are_the_models(gpu_lib, reads, monkeypatch, par):
    check_survivors(gpu_lib, reads["mix"], par, {}, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("par,env", EXACT_CASES, ids=_id)
def test_gpu_survivors_whatever_the_partition(gpu_lib, reads, monkeypatch, par, env):
    check_survivors(gpu_lib, reads["mix"], par, env, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("par,env,upper", LOOSE_CASES, ids=_id)
def test_gpu_counters_that_alias_only_add(gpu_lib, reads, monkeypatch, par, env, upper):
    check_survivors(gpu_lib, reads["mix"], par, env, monkeypatch, exact=False, upper=upper)


@pytest.mark.gpu
def test_gpu_long_pair_is_kept_whole(gpu_lib, reads, monkeypatch):
    check_survivors(gpu_lib, reads["long"], LONG, {}, monkeypatch)


@pytest.mark.gpu
def test_gpu_plan_is_what_the_first_pass_writes(gpu_lib, reads, monkeypatch):
    check_survivors(gpu_lib, reads["mix"], BASE, {}, monkeypatch, then_map=True)


@pytest.mark.gpu
def test_gpu_groups_of_queries(gpu_lib, reads, monkeypatch):
    check_survivors(gpu_lib, reads["mix"], BASE, GROUP_ENV, monkeypatch, groups=True)


@pytest.mark.gpu
def test_gpu_survivors_in_one_order_from_two_engines(gpu_lib, reads, monkeypatch):
    check_deterministic(gpu_lib, reads["mix"], BASE, [{}, {}], monkeypatch)
    check_deterministic(gpu_lib, reads["mix"], BASE, [dict(EXACT_ENVS[5]), dict(EXACT_ENVS[5])], monkeypatch)


@pytest.mark.gpu
def test_gpu_not_bucketed(gpu_lib, reads, monkeypatch):
    check_not_bucketed(gpu_lib, reads["mix"], monkeypatch)

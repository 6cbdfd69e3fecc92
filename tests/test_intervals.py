"""The stage between the chains and the table's region columns, at its own level: the per-part filter (k_split_ivl, the pair sort,
k_ivl_offsets, the room taken in the pool of persisted intervals, k_filter_redundant: lqcov_handle::filter_intervals, restating
filter_redundant_coords, lqmap.c:25-100) and pass 2 (k_reliable / lq_sweep in lqcov_handle::finish, restating
compute_reliable_region, lqutils.c:83-155), against the reference's own two functions run by `ref_harness intervals`
(oracle/ref_harness.c; replayed from tests/golden/ref_runs/ where oracle/_ref is not built; tests/test_oracle_vs_ref.py pins the
oracle's restatement to the same runs).

The way in: lqcov_debug_filter_intervals hands one part's intervals to filter_intervals, the function map_batch calls;
lqcov_accum_export_dev shows what is persisted after each part, lqcov_finish sweeps it, lqcov_accum_import_dev puts a set of
persisted intervals in front of lqcov_finish directly.

Queries: 130 random reads of 60-189 bases, all lengths different, so that the engine's order (longest first) is known: one thread
a query in 64 + 64 + 2.  The stage does not read the lengths.  tests.helpers.IVL_EMPTY are the queries without intervals: the
engine's positions 0, 63, 64, 129 under either order of the lengths, and two inside a block.

Inputs (made by tests.helpers.make_interval_cases, seed 83, and kept as made under tests/golden/intervals/, from where
tests.helpers.interval_cases reads them: the reference's recorded runs are keyed by their bytes; 13 415 intervals in all), three
parts each:
  mixed_c1, _c2, _c3, _c5 (-c 1, 2, 3, 5; 2 450 to 2 550 intervals): the same random intervals under every -c --
      crowded: 8 queries over 12 bases and 8 over 40, 6-40 intervals a part, lengths from {0, 1, 2, span/8, span/2}, 60 % medium:
        most events tie at a coordinate, the low three bits order them;
      ordinary: 2 queries over 3 000 bases and 2 over 200 000, 30-64 intervals a part;
      sparse: 57 queries of 0-2 intervals a part (neighbours with different numbers of intervals, queries that skip a part);
    and by hand, each on a query of its own --
      the quirk of lqmap.c:63 (decoded end minus *encoded* start): for s in 0..3 the lone medium interval [s, 8s + 2), which -c 1
        does not merge, and [max(s - 1, 0), 8s + 2) under [s, 8s + 5), which -c 2 does not merge, with the neighbours that close
        at 8s + 1 and 8s + 3, which are merged;
      markers against new intervals: part 0 makes the merged region [100, 200); part 1 brings an interval strictly inside it,
        equal to it, sharing either end, overhanging by one base on either side and on both -- medium, not medium, and -c
        medium copies (a second marker); part 2 one medium interval over it all.
  long_c3: one query of 1 800 intervals a part over 3 000 000 bases (the per-thread heapsort over 3 600 events a part, over what
      three parts persisted in pass 2) between neighbours of one and of two intervals, and a query of 30 identical intervals a part.
  growth_c3: a first part of 12 intervals leaves a pool of some 400 with intervals in it; the second part's 300 do not fit
      (info[1] == 1: grow_keep moves the earlier ones).

Checks, all exact: after every part the persisted intervals of every query, as a sorted multiset (slots are handed out by
atomicAdd), equal the reference's `V` lines of that part, and info[0] their number; after finish() rows()' regions equal the `R`
and `M` lines in order and the region columns of table_text() parse back to them; the final `V` set imported in shuffled order
into a fresh handle gives the same regions; the case run again with the lengths descending (the engine's order is the other
permutation) gives the same per query.

What the reference makes of these inputs (test_interval_inputs_have_teeth computes it from the reference's output and asserts
every kind is present; counted with the reference's functions through ref_harness):
  1 696 merged regions (markers); 5 122 intervals dropped as inside one; 132 closings of zero length in pass 2; 158 of the 520
  queries with intervals (six cases) end without a region; 202 have medium regions other than their regions; the 8 hand-made
  inputs of lqmap.c:63 make no marker and each of their 16 neighbours does; -c 1, 2 and 5 each change what the random intervals
  give under -c 3.

Which case notices which mutant (each seeded into a copy of the sources outside the repository, the emulator tests of this
module; `stage` = test_emulated_filter_and_regions and its twin with the lengths descending, `interleaved` = ..._threads_interleaved,
`import` = test_emulated_regions_of_imported_intervals):
  `med_start >> 3` in k_filter_redundant's mlen line: stage and interleaved, every mixed case and long_c3 -- mixed_c1 at the
      lone quirk intervals (query 23: the marker [2, 18) where the reference keeps the interval), mixed_c2 and the others at the
      crowded queries, whose merged regions of no bases the reference does mark (decoded minus encoded is not 0);
  scratch stride `lo * 2` in k_filter_redundant: interleaved alone, mixed_c1 and mixed_c3 (a neighbour's events land in the
      sweep: an interval too many).  Run thread after thread the emulator cannot see it: every thread is done with its scratch
      before the next one writes, which is what the interleaved runs are for;
  `>` for `>=` in the inside test: stage and interleaved, every case;
  the marker's `cov += min_cov - 1` (and its `-=`) left out of lq_sweep: stage, interleaved and import, every case but mixed_c1
      (min_cov - 1 is 0 there);
  the `> 0` length checks dropped in lq_sweep: stage, interleaved and import, every case but growth_c3;
  `q >= n_q` in k_ivl_offsets: the first emulator test ends the process (the last thread's offset is never written: the query
      at the engine's position 129 takes what lies there for its number of intervals);
  grow_keep keeping one interval fewer in filter_intervals: stage, growth_c3 (part 1: the last persisted interval of part 0 is
      lost in the move)."""
import numpy as np
import pytest

from longqc_amd import api
from tests import oracle_bind
from tests.helpers import IVL_EMPTY, IVL_N_QUERIES, interval_cases, parse_interval_dump, write_interval_case
from tests.test_chain_limits import _export

CASES = {c["name"]: c for c in interval_cases()}
_REF = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """name of a case -> (V, R, M) of the reference's run on it, run once a session"""
    d = tmp_path_factory.mktemp("intervals")

    def get(name):
        if name not in _REF:
            fn = str(d / (name + ".txt"))
            write_interval_case(CASES[name], fn)
            _REF[name] = parse_interval_dump(oracle_bind.ref_dump(["intervals", str(CASES[name]["min_cov"]), fn]))
        return _REF[name]
    return get


def queries(descending):
    """(names, reads, the engine's order of them): lengths 60 .. 189 in the caller's order, or 189 .. 60"""
    rng = np.random.default_rng(1273)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = 60 + np.arange(IVL_N_QUERIES)
    order = np.arange(IVL_N_QUERIES)[::-1]                      # longest first
    if descending:
        lens, order = lens[::-1], order[::-1]
    return ["q%03d" % i for i in range(IVL_N_QUERIES)], [acgt[rng.integers(0, 4, size=int(n))] for n in lens], order


def engine(lib, case, descending):
    p = api.Params()
    lib.lqcov_params_default(p)
    p.min_coverage = case["min_cov"]
    eng = api.Engine(p, 0, lib=lib)
    try:
        names, seqs, order = queries(descending)
        eng.set_queries(names, seqs)
        perm = eng.query_order().astype(np.int64)               # perm[i]: the caller's index of the engine's i-th query
        assert perm.tolist() == order.tolist()
        for pos in (0, 63, 64, 129):
            assert int(perm[pos]) in IVL_EMPTY
    except Exception:
        eng.close()
        raise
    inv = np.empty(IVL_N_QUERIES, dtype=np.int64)
    inv[perm] = np.arange(IVL_N_QUERIES)
    return eng, perm, inv


def per_query(iv, perm):
    """intervals [n, 3] in the engine's numbering -> {query in the caller's order: sorted [(start, end)]}"""
    out = {}
    for q, s, e in iv.tolist():
        out.setdefault(int(perm[q]), []).append((s, e))
    return {q: sorted(v) for q, v in out.items()}


def first_diff(got, want):
    for q in sorted(set(got) | set(want)):
        if got.get(q, []) != want.get(q, []):
            return "query %d: engine %r, reference %r" % (q, got.get(q, []), want.get(q, []))
    return ""


def table_columns(text):
    """the region columns of the table, in row order: [(regions, medium regions)], "0" = none"""
    def col(s):
        return [] if s == "0" else [[int(x) for x in r.split("-")] for r in s.split(",")]
    return [(col(f[3]), col(f[4])) for f in (line.split("\t") for line in text.splitlines())]


def check_regions(eng, R, M, what):
    eng.finish()
    rows = eng.rows()
    cols = table_columns(eng.table_text())
    assert len(rows) == len(cols) == IVL_N_QUERIES
    for j, r in enumerate(rows):
        want_r, want_m = [list(x) for x in R.get(j, [])], [list(x) for x in M.get(j, [])]
        assert r["regs"] == want_r, "%s, query %d: regions %r, the reference has %r" % (what, j, r["regs"], want_r)
        assert r["mregs"] == want_m, "%s, query %d: medium regions %r, the reference has %r" % (what, j, r["mregs"], want_m)
        # (a row without regions prints neither list: minimap2-coverage.c:596-604)
        assert cols[j] == (want_r, want_m if want_r else []), "%s, query %d: the table has %r" % (what, j, cols[j])


def run_stage(lib, on_device, name, ref, descending=False):
    """every part through lqcov_debug_filter_intervals, then finish(): the `V` lines after every part, the regions at the end"""
    case = CASES[name]
    V, R, M = ref(name)
    rng = np.random.default_rng(97)
    eng, perm, inv = engine(lib, case, descending)
    try:
        n_before = 0
        for part, ivs in enumerate(case["parts"]):
            a = np.array(ivs, dtype=np.int64).reshape(-1, 3)
            a[:, 0] = inv[a[:, 0]]
            a = a[rng.permutation(a.shape[0])].astype(np.uint32)   # (any order: the stage sorts by query)
            n_pv, grew = eng.debug_filter_intervals(a)
            got = per_query(_export(eng, on_device)[4], perm)
            assert got == V[part], "%s part %d, %s" % (name, part, first_diff(got, V[part]))
            assert n_pv == sum(len(v) for v in V[part].values())
            if case["grows"] == part:
                assert n_before > 0 and grew, "part %d was to move %d persisted intervals to a larger pool" % (part, n_before)
            n_before = n_pv
        check_regions(eng, R, M, "%s, lengths %s" % (name, "descending" if descending else "ascending"))
    finally:
        eng.close()


def run_import(lib, on_device, name, ref):
    """the final `V` set through lqcov_accum_import_dev on a fresh handle, in shuffled order, then finish()"""
    case = CASES[name]
    V, R, M = ref(name)
    eng, perm, inv = engine(lib, case, False)
    try:
        iv = np.array([(inv[q], s, e) for q, v in V[-1].items() for s, e in v], dtype=np.uint32).reshape(-1, 3)
        iv = np.ascontiguousarray(iv[np.random.default_rng(98).permutation(iv.shape[0])])
        n_q, n_cnt, n_ivl = eng.accum_sizes()
        assert n_q == IVL_N_QUERIES and n_ivl == 0
        arrs = [np.zeros(n_q, dtype=np.uint64), np.zeros(n_q, dtype=np.uint64), np.zeros(n_q, dtype=np.float32), np.zeros(n_q, dtype=np.uint32),
                np.zeros(max(n_cnt, 1), dtype=np.uint32), iv if iv.shape[0] else np.zeros((1, 3), dtype=np.uint32)]
        if on_device:                                           # the real library copies device to device
            import torch
            keep = [torch.from_numpy(a.view(np.uint8).reshape(-1)).to("cuda:0") for a in arrs]
            ptrs = [t.data_ptr() for t in keep]
        else:                                                   # the emulator's device memory is the host's
            ptrs = [a.ctypes.data for a in arrs]
        eng.accum_import(*ptrs, iv.shape[0])
        check_regions(eng, R, M, "%s imported" % name)
    finally:
        eng.close()


# ---- what the inputs reach, from the reference's output ----

def sweep(v, min_cov):
    """compute_reliable_region (lqutils.c:83-155) on a query's persisted intervals -> (regions, medium regions, closings of
    either kind dropped because their length is 0)"""
    u32 = 0xffffffff
    start = cov = med_start = med_cov = zero = 0
    regs, mregs = [], []

    def close(lst, st, e):
        if ((e >> 3) - st) & u32:
            lst.append((st, e >> 3))
            return 0
        return 1
    for e in sorted(x for iv in v for x in iv):
        old_cov, old_med = cov, med_cov
        d = -1 if e & 1 else 1
        cov = (cov + d) & u32
        if e & 2:
            if e & 4:
                med_cov = (med_cov + d * min_cov) & u32
                cov = (cov + d * (min_cov - 1)) & u32
            else:
                med_cov = (med_cov + d) & u32
        if old_cov < min_cov <= cov:
            start = e >> 3
            if old_med < min_cov <= med_cov:
                med_start = e >> 3
        elif old_cov >= min_cov > cov:
            zero += close(regs, start, e)
            if old_med >= min_cov > med_cov:
                zero += close(mregs, med_start, e)
        elif old_med < min_cov <= med_cov:
            med_start = e >> 3
        elif old_med >= min_cov > med_cov:
            zero += close(mregs, med_start, e)
    return regs, mregs, zero


def n_markers(v):
    return sum(1 for s, _ in v if s & 4)


def test_interval_inputs_have_teeth(ref):
    """non-vacuity, from the reference's output alone: markers are made, intervals are dropped as inside a merged region, closings
    are dropped for zero length, queries end without a region, medium regions differ from the regions, every hand-made input of
    lqmap.c:63 makes no marker while its neighbours do, and every -c changes what the same intervals give under -c 3"""
    tot = dict(markers=0, dropped=0, zero=0, queries=0, no_region=0, m_differs=0)
    for name, case in CASES.items():
        V, R, M = ref(name)
        with_intervals = set()
        for part, ivs in enumerate(case["parts"]):
            n_in = {}
            for q, _, _ in ivs:
                n_in[q] = n_in.get(q, 0) + 1
            with_intervals |= set(n_in)
            for q, n in n_in.items():
                now, before = V[part].get(q, []), V[part - 1].get(q, []) if part else []
                made = n_markers(now) - n_markers(before)
                kept = len(now) - len(before) - made
                assert 0 <= kept <= n and made >= 0
                tot["markers"] += made
                tot["dropped"] += n - kept
        for q in sorted(with_intervals):
            regs, mregs, zero = sweep(V[-1].get(q, []), case["min_cov"])
            assert (regs, mregs) == (R.get(q, []), M.get(q, [])), "%s, query %d: the sweep restated here is not the reference's" % (name, q)
            tot["zero"] += zero
            tot["queries"] += 1
            tot["no_region"] += q not in R
            tot["m_differs"] += R.get(q, []) != M.get(q, [])
        assert not set(R) - with_intervals and not set(M) - with_intervals and not with_intervals & set(IVL_EMPTY)
        for q, (form, s, d) in case["quirk"].items():          # (a quirk query's intervals are all in part 0)
            if form == case["min_cov"]:
                assert (n_markers(V[0].get(q, [])) == 0) == (d == 0), "%s: form %d, s %d, end %+d" % (name, form, s, d)
    print("\nreference counts: %(markers)d merged regions (markers), %(dropped)d intervals dropped as inside one, %(zero)d closings of zero length, "
          "%(no_region)d of %(queries)d queries with intervals end without a region, %(m_differs)d with medium regions other than the regions" % tot)
    assert tot["markers"] and tot["dropped"] and tot["zero"] and tot["no_region"] and tot["m_differs"]
    assert sum(1 for c in CASES.values() for f, _, d in c["quirk"].values() if f == c["min_cov"] and d == 0) == 8
    V3, R3, M3 = ref("mixed_c3")
    for c in (1, 2, 5):
        Vc, Rc, Mc = ref("mixed_c%d" % c)
        rq = CASES["mixed_c3"]["random"]
        assert any((Vc[-1].get(q), Rc.get(q), Mc.get(q)) != (V3[-1].get(q), R3.get(q), M3.get(q)) for q in rq), "-c %d gives what -c 3 gives" % c


# ---- emulator ----

@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_filter_and_regions(emu_lib, ref, name, monkeypatch):
    monkeypatch.delenv("LQ_EMU_ORDER", raising=False)
    run_stage(emu_lib, False, name, ref)


@pytest.mark.parametrize("name", ["long_c3", "mixed_c1", "mixed_c3"])
def test_emulated_filter_and_regions_threads_interleaved(emu_lib, ref, name, monkeypatch):
    """the threads of a block take turns at their atomics (the emulator runs them one after the other otherwise: a thread that
    writes into its neighbour's scratch would do no harm)"""
    monkeypatch.setenv("LQ_EMU_ORDER", "random:5")
    run_stage(emu_lib, False, name, ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_regions_of_imported_intervals(emu_lib, ref, name):
    run_import(emu_lib, False, name, ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_filter_and_regions_lengths_descending(emu_lib, ref, name, monkeypatch):
    monkeypatch.delenv("LQ_EMU_ORDER", raising=False)
    run_stage(emu_lib, False, name, ref, descending=True)


# ---- MI355X ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_filter_and_regions(gpu_lib, ref, name):
    run_stage(gpu_lib, True, name, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_regions_of_imported_intervals(gpu_lib, ref, name):
    run_import(gpu_lib, True, name, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_filter_and_regions_lengths_descending(gpu_lib, ref, name):
    run_stage(gpu_lib, True, name, ref, descending=True)

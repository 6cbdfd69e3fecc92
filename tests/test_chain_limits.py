"""Chaining with the gap limit (-g, max_gap), the skip limit (-s, max_chain_skip) and the band (bw) biting, compared stage by
stage with the oracle's `chains` dump: mid_occ, every chain, lambda / lambda2, the overlap intervals after
filter_redundant_coords (`V` lines) and every non-zero match counter (`N` lines), per query.  The rest of the suite runs these
three limits at their defaults (10000, 25, 500), where reads of 1-10 kb almost never reach them.

Inputs
  (a) tests/golden/adv_all.fa.gz / adv_sub.fq.gz (690 targets, 2580 oracle chains at the defaults, 1453 of them longer than
      64 anchors): -g 100 -> 2919 chains, -g 300 -> 2597, -s 0 -> 2579.
  (b) tests.helpers.limits_dataset(): a 12-kb random genome; every 2 kb a tandem repeat (period 40-300 bases, up to 9 copies
      that differ in 1 % of their bases); one 500-base segment copied to two other places, one of them reverse-complemented;
      19 targets of 1-4 kb and 4 queries of 1.5-4 kb cut at random places and strands with 2 % errors; one target of 6.5 kb
      with a query of 6.8 kb over it at 0.5 % errors (one run of about 1900 collinear anchors); 3 queries of 2-3 kb with 13 %
      errors (sparse anchors: the best predecessor is often the only one in reach, now and then exactly max_gap away); 10
      targets that copy 400 bases of the long query's stretch exactly and go on for 20-24 bases beyond a deletion of 70-97
      (two or three anchors whose diagonal is 70-97 off: within a band of 100, beyond a diagonal bin of 64).  The oracle's
      chains (all / longer than 64 anchors / longest) with -k 12 -w 5 -m 40:
          defaults 495 / 192 / 1920
          -g 60    808 / 251 / 1920     -g 150  608 / 245 / 1920     -g 250  598 / 246 / 1920     -g 1000  495 / 192 / 1920
          -s 0     541 / 159 / 1671     -s 1    540 / 165 / 1735     -s 2    534 / 169 / 1735     -s 3     547 / 166 / 1920
          bw 0     1675 / 153 / 524     bw 8    642 / 264 / 1920     bw 64   635 / 264 / 1920     bw 100   573 / 241 / 1920
      Each of these changes the dump of seven or all eight queries against the default (-g 1000: of two), -s 1, 2 and 3
      included: the dense anchors of low-error reads make a scan meet more than three already-chained predecessors all the
      time.  About 64 minimizers of -k 12 -w 5 span some 200 bases, so -g 150 / 250 / 1000 bracket the switch between
      k_chain_wave's `far` ballot (the window of 64 older anchors reaches beyond max_gap) and its walk through memory (more
      than 64 inside).  bw 100 is there for the pre-filter: at a power-of-two band (0, 8, 64) bins one bit too narrow still
      keep every two anchors that interact in neighbouring bins; at 100 they do not.

The reference's binary takes -g and -s and has no option for bw (map.c:20 fixes it at 500): the bw cases compare the engine
with the oracle only (oracle CLI: --bw N); -g and -s are pinned through the reference's tables below and in
tests/test_oracle_vs_ref.py.  Both chain kernels (k_chain, k_chain_wave) and the klib-order second pass record their chains
under debug bit 0, so every case compares the chain list too.

The non-vacuity conditions (every non-default value changes the oracle's dump; one of -s 1..3 differs from -s 25; one bw
below 500 differs from 500; (b) has chains on both sides of 64 anchors) are computed from the oracle's dumps alone and are
asserted in test_limits_inputs_have_teeth.

Which case notices which off-by-one (each seeded into a copy of the sources, emulator): `>= max_dist` in k_chain's `st` advance:
-g 60 in the default environment and with LQCOV_CHAIN_CAP=256 (q007, stage and table); the same in k_chain_wave's `far`
ballot: -g 60 (stage and table); `>= max_skip` in k_chain: -s 1, 2, 3 with LQCOV_CHAIN_CAP=256 + LQCOV_CHAIN_WAVE_MIN=257, where
k_chain takes every run of up to 256 anchors (by default it sees runs below 48, where the skip limit changed nothing here);
the same in lq_wave_replay: every stage case but -s 0 and the bw ones, the table only at the defaults; dp.dshift one
smaller: bw 100 (q004, the chains that lose their anchors beyond the deletion); counters exported one place off: every stage
case, no table."""
import os

import numpy as np
import pytest

from longqc_amd import api
from tests import oracle_bind
from tests.conftest import GOLDEN
from tests.helpers import ONT, limits_dataset, parse_chain_dump, read_fastx, run_main, slow_emu

DEFAULTS = {"max_gap": 10000, "max_chain_skip": 25, "bw": 500, "min_cnt": 3, "min_chain_score": 40}
FLAG = {"max_gap": "-g", "max_chain_skip": "-s", "bw": "--bw", "min_cnt": "-n", "min_chain_score": "-m"}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (targets, queries): (a) the committed adversarial fixtures, (b) the seeded repeat-rich set"""
    return {"adv": (os.path.join(GOLDEN, "adv_all.fa.gz"), os.path.join(GOLDEN, "adv_sub.fq.gz")),
            "rr": limits_dataset(tmp_path_factory.mktemp("limits"))}


def _flags(par):
    return [x for k in sorted(par) if par[k] != DEFAULTS[k] for x in (FLAG[k], str(par[k]))]


_DUMPS, _READS = {}, {}


def oracle_chains(files, par):
    """(text, mid_occ, {query index in file order: ...}) of the oracle's `chains` dump; one run per (files, parameters) and session"""
    par = dict(DEFAULTS, **par)
    key = (files, tuple(sorted(par.items())))
    if key not in _DUMPS:
        txt = oracle_bind.dump("chains", ["-k", "12", "-w", "5", "-p", "160", "-q", "160", "-l", "0"] + [x for k in sorted(par) for x in (FLAG[k], str(par[k]))], list(files))
        _DUMPS[key] = (txt,) + parse_chain_dump(txt)
    return _DUMPS[key]


def _reads(fn):
    if fn not in _READS:
        _READS[fn] = read_fastx(fn)
    return _READS[fn]


def _first_diff(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "item %d: engine %r, oracle %r" % (k, g, w)
    k = min(len(got), len(want))
    return "item %d: engine %r, oracle %r (%d against %d items)" % (k, got[k] if k < len(got) else None, want[k] if k < len(want) else None, len(got), len(want))


def _export(eng, on_device):
    """the accumulators of lqcov_accum_export_dev as host arrays: (lambda, lambda2, counters, counter_owner, intervals[n, 3])"""
    n_q, n_cnt, n_ivl = eng.accum_sizes()
    shapes = [((n_q,), np.uint64), ((n_q,), np.uint64), ((n_q,), np.float32), ((n_q,), np.uint32), ((n_cnt,), np.uint32), ((n_cnt,), np.uint32), ((n_ivl, 3), np.uint32)]
    if on_device:                                               # the real library copies device to device
        import torch
        tt = {np.uint64: torch.int64, np.float32: torch.float32, np.uint32: torch.int32}
        bufs = [torch.zeros(max(int(np.prod(s)), 1), dtype=tt[t], device="cuda:0") for s, t in shapes]
        eng.accum_export(*[b.data_ptr() for b in bufs])
        out = [b.cpu().numpy().view(t)[:int(np.prod(s))].reshape(s) for b, (s, t) in zip(bufs, shapes)]
    else:                                                       # the emulator's device memory is the host's
        bufs = [np.zeros(max(int(np.prod(s)), 1), dtype=t) for s, t in shapes]
        eng.accum_export(*[b.ctypes.data for b in bufs])
        out = [b[:int(np.prod(s))].reshape(s) for b, (s, t) in zip(bufs, shapes)]
    return out[0], out[1], out[4], out[5], out[6]


def check_stages(lib, files, par, env, monkeypatch, on_device=False):
    """One part built through the engine with set_debug(1) and the Params override `par`, mapped under the environment `env`,
    against the oracle's `chains` dump of the same files and parameters; an AssertionError names the query and the first item
    that differs."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, mid, want = oracle_chains(files, par)
    tn, ts, _ = _reads(files[0])
    qn, qs, qq = _reads(files[1])
    p = api.Params()
    lib.lqcov_params_default(p)
    p.no_self = 1; p.min_ovlp = 0; p.min_score_med = 160; p.min_score_good = 160
    for k, v in par.items():
        assert k in DEFAULTS, k
        setattr(p, k, v)
    eng = api.Engine(p, 0, lib=lib)
    try:
        eng.set_debug(1)
        eng.set_queries(qn, qs, qq)
        pt = eng.part_begin()
        eng.part_add_targets(pt, tn, ts)
        eng.part_build(pt)
        assert eng.mid_occ == mid, "mid_occ: engine %d, oracle %d" % (eng.mid_occ, mid)
        eng.part_map(pt)
        eng.sync()
        ch = eng.chains()
        perm = eng.query_order().astype(np.int64)               # perm[engine index] = index in the file
        off = eng.counter_offsets().astype(np.int64)
        lam, lam2, cnts, owner, ivl = _export(eng, on_device)
        eng.finish()
        rows = eng.rows()
    finally:
        eng.close()
    assert sorted(perm.tolist()) == list(range(len(qn)))
    assert off[0] == 0 and off[-1] == cnts.shape[0] and np.all(np.diff(off) >= 0)
    assert np.array_equal(owner, np.repeat(np.arange(len(qn), dtype=np.uint32), np.diff(off))), "counter_owner does not follow counter_offsets"
    assert sorted(want) == list(range(len(qn)))
    by_q = {}
    for r in ch:
        by_q.setdefault(int(r[0]), []).append(tuple(int(v) for v in r[1:]))
    ivl_by_e = {}
    for e, s, t in ivl.tolist():
        ivl_by_e.setdefault(e, []).append((s, t))
    for e, qi in enumerate(perm.tolist()):
        w = want[qi]
        assert w["name"] == qn[qi]
        got = sorted(by_q.get(qi, []))                          # (rid, rev, score, cnt, qs, qe, rs, re)
        exp = sorted(w["chains"])
        assert got == exp, "%s: chains, %s" % (w["name"], _first_diff(got, exp))
        assert (int(lam[e]), int(lam2[e])) == (w["lambda_"], w["lambda2"]), "%s: exported lambda, lambda2 %d, %d; oracle %d, %d" % (w["name"], lam[e], lam2[e], w["lambda_"], w["lambda2"])
        assert (rows[qi]["lambda_"], rows[qi]["lambda2"]) == (w["lambda_"], w["lambda2"]), "%s: lambda, lambda2 of the row" % w["name"]
        got = sorted(ivl_by_e.get(e, []))                       # encoded as the reference keeps them: position << 3 | flags
        exp = sorted(w["ivl"])
        assert got == exp, "%s: intervals (position, flags), %s" % (w["name"], _first_diff([((s >> 3, s & 7), (t >> 3, t & 7)) for s, t in got], [((s >> 3, s & 7), (t >> 3, t & 7)) for s, t in exp]))
        c = cnts[off[e]:off[e + 1]]
        got = [(int(j), int(c[j])) for j in np.flatnonzero(c)]
        exp = sorted(w["cnt"].items())
        assert not exp or exp[-1][0] < c.shape[0], "%s: the oracle counts minimizer %d, the engine has %d counters" % (w["name"], exp[-1][0], c.shape[0])
        assert got == exp, "%s: counters (minimizer, count), %s" % (w["name"], _first_diff(got, exp))


def check_table(lib, files, flags):
    argv = ONT + flags + list(files)
    want = oracle_bind.ref_table(argv) if oracle_bind.have_ref() else oracle_bind.table(argv)
    rc, out, err = run_main(lib, argv)
    assert rc == 0, err
    if out != want:
        for g, w in zip(out.splitlines(), want.splitlines()):
            assert g == w, "row of %s: engine %r, reference %r" % (w.split("\t")[0], g, w)
    assert out == want


# ---- the cases ----------------------------------------------------------------------------------------------------------------
GRID = {
    "adv": [{}, {"max_gap": 100}, {"max_gap": 300}, {"max_chain_skip": 0}],      # (with -g 100 or 300, -s 0 changes nothing here: no combination)
    "rr": [{}, {"max_gap": 60}, {"max_gap": 150}, {"max_gap": 250}, {"max_gap": 1000},
           {"max_chain_skip": 0}, {"max_chain_skip": 1}, {"max_chain_skip": 2}, {"max_chain_skip": 3},
           {"bw": 0}, {"bw": 8}, {"bw": 64}, {"bw": 100},
           {"max_gap": 250, "max_chain_skip": 1}, {"max_gap": 150, "bw": 8}, {"max_chain_skip": 2, "bw": 64}],
}
PATH_PARS = [{}, {"max_gap": 250}, {"max_chain_skip": 1}]       # defaults, gap-limited, skip-limited
C256 = {"LQCOV_CHAIN_CAP": "256", "LQCOV_CHAIN_WAVE_MIN": "257"}    # wave_min = min(cap + 1, LQCOV_CHAIN_WAVE_MIN): k_chain<256> takes every run of up to 256 anchors
PATH_ENVS = [{"LQCOV_CHAIN_WAVE_MIN": "3"}, {"LQCOV_CHAIN_CAP": "64", "LQCOV_CHAIN_WAVE_MIN": "200"}, C256, {"LQCOV_TIES": "klib"}, {"LQCOV_SORT": "klib"}]
TABLE_FLAGS = {"adv": [["-g", "300"], ["-s", "0"]], "rr": [["-g", "300"], ["-s", "1"]]}


def _pid(par):
    return "_".join(_flags(par)).replace("--", "").replace("-", "") or "defaults"


def _eid(env):
    return "+".join("%s=%s" % kv for kv in sorted(env.items())) or "default_env"


GRID_CASES = [(name, par) for name in ("adv", "rr") for par in GRID[name]]
PATH_CASES = [("rr", par, env) for env in PATH_ENVS for par in PATH_PARS] + [("rr", {"max_gap": 60}, C256), ("rr", {"max_chain_skip": 3}, C256)] + [("adv", par, env) for env in PATH_ENVS for par in ({"max_gap": 300}, {"max_chain_skip": 0})]
TABLE_CASES = [(name, fl) for name in ("adv", "rr") for fl in TABLE_FLAGS[name]]


def test_limits_inputs_have_teeth(inputs):
    """the non-vacuity conditions of the module docstring, from the oracle's dumps alone"""
    used = {name: list(GRID[name]) for name in GRID}
    for name, par, _ in PATH_CASES:
        used[name].append(par)
    for name, pars in used.items():
        for par in pars:
            for k in par:
                less = {a: b for a, b in par.items() if a != k}
                assert oracle_chains(inputs[name], par)[0] != oracle_chains(inputs[name], less)[0], (name, par, "the same dump with %s at its default" % k)
    for name, flags in TABLE_CASES:
        argv = ONT + list(inputs[name])
        assert oracle_bind.table(ONT + flags + list(inputs[name])) != oracle_bind.table(argv), (name, flags)
    rr = inputs["rr"]
    assert any(oracle_chains(rr, {"max_chain_skip": s})[0] != oracle_chains(rr, {})[0] for s in (1, 2, 3))
    assert any(oracle_chains(rr, {"bw": b})[0] != oracle_chains(rr, {})[0] for b in (0, 8, 64))
    for par in GRID["rr"]:
        cnt = [c[3] for q in oracle_chains(rr, par)[2].values() for c in q["chains"]]
        assert max(cnt) > 64 and min(cnt) < 64, par


# The emulator's default run keeps, on (b), the defaults, the cases around each boundary, the default parameters under every
# kernel path and the two cases that reach k_chain's boundaries; the others take their 30 s (adv) or 9 s (rr) only with
# LQCOV_SLOW_TESTS=1.  The -m gpu twins below run every case.
_QUICK_GRID = [("rr", p) for p in ({}, {"max_gap": 60}, {"max_gap": 150}, {"max_gap": 250}, {"max_chain_skip": 0}, {"max_chain_skip": 1}, {"bw": 0}, {"bw": 8}, {"bw": 100})]
_QUICK_PATH = [("rr", {}, e) for e in PATH_ENVS] + [("rr", {"max_gap": 250}, PATH_ENVS[0]), ("rr", {"max_chain_skip": 1}, C256), ("rr", {"max_gap": 60}, C256)]


def _emu(cases, quick):
    return [c if c in quick else pytest.param(*c, marks=slow_emu) for c in cases]


def _id(v):
    return v if isinstance(v, str) else "".join(v) if isinstance(v, list) else _eid(v) if any(k.startswith("LQ") for k in v) else _pid(v)


@pytest.mark.parametrize("name,par", _emu(GRID_CASES, _QUICK_GRID), ids=_id)
def test_emulated_stages_at_the_limits(emu_lib, inputs, monkeypatch, name, par):
    check_stages(emu_lib, inputs[name], par, {}, monkeypatch)


@pytest.mark.parametrize("name,par,env", _emu(PATH_CASES, _QUICK_PATH), ids=_id)
def test_emulated_stages_on_every_kernel_path(emu_lib, inputs, monkeypatch, name, par, env):
    """k_chain_wave for every run of three anchors and more; k_chain<64> for the runs of up to 64 anchors and k_chain_wave for the
    rest (the engine clamps LQCOV_CHAIN_WAVE_MIN to the LDS budget + 1); k_chain<256> for every run of up to 256 anchors, where
    its `st` window and its skip break decide chains; every run through the klib-order second pass; every query sorted in
    klib's passes"""
    check_stages(emu_lib, inputs[name], par, env, monkeypatch)


def test_emulated_stages_with_threads_in_descending_order(emu_lib, inputs, monkeypatch):
    check_stages(emu_lib, inputs["rr"], {}, {"LQ_EMU_ORDER": "reverse"}, monkeypatch)


@pytest.mark.parametrize("name,flags", _emu(TABLE_CASES, [c for c in TABLE_CASES if c[0] == "rr"]), ids=_id)
def test_emulated_tables_at_the_limits(emu_lib, inputs, name, flags):
    """-g / -s through lqcov_main's argv against the reference's binary (the oracle where it is not built)"""
    check_table(emu_lib, inputs[name], flags)


@pytest.mark.gpu
@pytest.mark.parametrize("name,par", GRID_CASES, ids=_id)
def test_gpu_stages_at_the_limits(gpu_lib, inputs, monkeypatch, name, par):
    check_stages(gpu_lib, inputs[name], par, {}, monkeypatch, on_device=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,par,env", PATH_CASES, ids=_id)
def test_gpu_stages_on_every_kernel_path(gpu_lib, inputs, monkeypatch, name, par, env):
    check_stages(gpu_lib, inputs[name], par, env, monkeypatch, on_device=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", TABLE_CASES, ids=_id)
def test_gpu_tables_at_the_limits(gpu_lib, inputs, name, flags):
    check_table(gpu_lib, inputs[name], flags)

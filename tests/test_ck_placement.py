"""Where a level's kernels run (engine.cpp sort_batch, add_lane): the level's streaming kernels on the lane's own stream, the token
walkers on two streams confined to a quarter of the CUs -- the checkpointed walks behind their solvers (k_ck_plan, k_ck_tilehist,
k_ck_tilescan, k_ck_phases, k_ck_solve; k_ck_chain256) on the first, the whole walks of the shorter size classes on the second.
Three streams then work on one level at once, and what keeps them apart is three events:

  ev_w0  recorded on the lane's stream once the level's digits, histograms, bucket starts and class lists are written (k_rs_hist,
         k_sort_classify, k_sort_two).  Both walker streams wait for it; the checkpoint buffers are sized before it.
  ev_w1, ev_w2  recorded behind the walks of the first / second walker stream.  The lane's stream waits for both before
         k_rs_scatter reads the destinations and k_rs_children makes the next level's sub-arrays; the next level's ev_w0 comes
         later on that stream, so its solvers overwrite the checkpoint buffers only after this level's walk has read them.
  (The solvers were also measured on the lane's own stream behind an event of their own -- add_lane's comment; this file's cases
  are what that arrangement was checked with.)

A missing wait shows as a wrong order only when the streams happen to overlap that way, so the cases here make every stream busy
in the same level and repeat the call: one level holds, in four queries, checkpointed sub-arrays (longest two size classes),
sub-arrays of each of the three whole-walk classes, and two-bucket sub-arrays; a fifth query of distinct keys keeps the parallel
sort busy on the lane's second stream meanwhile.  LQCOV_WALK_SHIFT=5: class caps 128 / 512 / 2048 / 4992, checkpoint units 2048
and 256, 24 500 anchors.

  geometry (targets, longest)   the level     digits there     solver                      checkpointed walker     whole walkers
  400000, 3000                  48            rid >> 16: 7     k_ck_prefix, k_ck_solve     k_sort_walk_reg<1>ck    k_sort_walk_reg<1>, lds
  40000, 3000                   40            rid >> 8: 39     k_ck_chain256               k_sort_walk_solo_ck     k_sort_walk_solo, lds

Asserted: from the input, that the level holds those kinds of sub-array in at least three queries, with at most 16 / more than 16
digits in the checkpointed ones; from stage_times(), call by call, that the solver, the checkpointed walker, the whole walkers
and k_sort_two ran; every query's anchors equal lqo_sort_128x of its emitted ones; three calls on one handle give the same
bytes."""
import numpy as np
import pytest

from tests.test_anchor_sort import MARK, RS_MIN, U32, engine, first_diff, mark_exact, model_of

SHIFT = 5
CAPS = [4096 >> SHIFT, 16384 >> SHIFT, 65536 >> SHIFT, 159744 >> SHIFT]          # WalkCaps under LQCOV_WALK_SHIFT
# name -> (targets, longest target, the level's shift, bits of rid below the level's digit, digits of a general sub-array, stages)
GEOM = {
    "few_buckets": (400000, 3000, 48, 16, list(range(7)),
                    ["k_sort_two", "k_ck_prefix", "k_ck_solve", "k_sort_walk_reg<1>ck", "k_sort_walk_reg<1>", "k_sort_walk_lds<16384>", "k_sort_walk_lds<4096>"]),
    "many_buckets": (40000, 3000, 40, 8, list(range(2, 156, 4)),
                     ["k_sort_two", "k_ck_chain256", "k_sort_walk_solo_ck", "k_sort_walk_solo", "k_sort_walk_lds<16384>", "k_sort_walk_lds<4096>"]),
}
# the klib queries: (anchors, general or two-bucket) of strand 0 and of strand 1
LAYOUT = [((9000, "g"), (100, "g")), ((3000, "g"), (300, "g")), ((1000, "g"), (400, "t")), ((3000, "t"), (5500, "g"))]
N_PLAIN = 2200
_BATCHES = {}


def sub_array(rng, n, strand, digits, low_bits, max_len):
    """n keys of one strand whose digit at the level takes exactly the values `digits`; a pool of n / 48 targets and 12 positions,
    so a key occurs four times on average and no (strand, target) group outgrows the insertion sort's 64 by much"""
    low = 6000 if low_bits == 16 else 256                       # (the last digit's targets end early: 400000 - 6 * 65536, 40000 - 156 * 256)
    pool = np.unique(rng.choice(np.asarray(digits, dtype=np.uint64), size=n // 48 + 4) << np.uint64(low_bits) | rng.integers(0, low, size=n // 48 + 4, dtype=np.uint64))
    rid = rng.choice(pool, size=n)
    rid[:len(digits)] = (np.asarray(digits, dtype=np.uint64) << np.uint64(low_bits)) | (rid[:len(digits)] & np.uint64((1 << low_bits) - 1))   # every digit occurs
    pos = rng.choice(np.concatenate([rng.integers(0, 256, size=6, dtype=np.uint64), rng.integers(0, max_len, size=6, dtype=np.uint64)]), size=n)
    return (np.uint64(strand) << np.uint64(63)) | (rid << U32) | pos


def batch_of(name):
    """one batch per geometry with its model, made once and never changed"""
    if name not in _BATCHES:
        n_targets, max_len, shift, low_bits, digits, _ = GEOM[name]
        rng = np.random.default_rng(4800 + shift)
        xs = []
        for q, strands in enumerate(LAYOUT):
            parts = []
            for strand, (n, kind) in enumerate(strands):
                d = digits if kind == "g" else [digits[1 + q], digits[-1 - q]]
                parts.append(sub_array(rng, n, strand, d, low_bits, max_len))
            xs.append(rng.permutation(np.concatenate(parts)))
        plain = np.zeros(0, dtype=np.uint64)
        while plain.shape[0] < N_PLAIN:
            plain = np.unique(np.concatenate([plain, (rng.integers(0, 2, size=N_PLAIN, dtype=np.uint64) << np.uint64(63))
                                              | (rng.integers(0, n_targets, size=N_PLAIN, dtype=np.uint64) << U32) | rng.integers(0, max_len, size=N_PLAIN, dtype=np.uint64)]))
        xs.append(rng.permutation(plain)[:N_PLAIN])
        off = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int64)
        em = np.zeros((int(off[-1]), 2), dtype=np.uint64)
        em[:, 0] = np.concatenate(xs)
        em[:, 1] = (rng.integers(1, 29, size=em.shape[0], dtype=np.uint64) << U32) | np.arange(em.shape[0], dtype=np.uint64)
        for q, x in enumerate(xs):
            em[off[q]:off[q + 1], 1] |= np.where(mark_exact(x), MARK, np.uint64(0))
        b = dict(em=em, off=off, klib=np.array([1] * len(LAYOUT) + [0], dtype=np.uint32), n_targets=n_targets, max_len=max_len)
        assert int(np.max((em[:, 0] >> U32) & np.uint64(0x7fffffff))) < n_targets
        b["model"] = model_of(em, off)
        em.setflags(write=False); b["model"].setflags(write=False)
        _BATCHES[name] = b
    return _BATCHES[name]


def level_holds(b, shift):
    """-> {kind: [(query, buckets), ...]} for the sub-arrays of more than 64 anchors at the level on `shift`: "two", "walk0" ..
    "walk2" (whole walks by size class), "ck" (the two longest classes)"""
    out = {}
    for q in np.flatnonzero(b["klib"]):
        x = b["em"][b["off"][q]:b["off"][q + 1], 0]
        above = x >> np.uint64(shift + 8)
        for a in np.unique(above):
            s = x[above == a]
            nz = np.unique((s >> np.uint64(shift)) & np.uint64(0xff)).shape[0]
            if s.shape[0] <= RS_MIN or nz < 2:
                continue
            c = sum(s.shape[0] > cap for cap in CAPS)
            out.setdefault("two" if nz == 2 else "ck" if c >= 3 else "walk%d" % c, []).append((int(q), nz))
    return out


def run_case(lib, name, monkeypatch):
    n_targets, max_len, shift, low_bits, digits, stages = GEOM[name]
    b = batch_of(name)
    holds = level_holds(b, shift)
    assert set(holds) == {"two", "walk0", "walk1", "walk2", "ck"}, sorted(holds)
    assert len({q for v in holds.values() for q, _ in v}) >= 3 and len(holds["ck"]) >= 3 and len(holds["two"]) >= 2
    if name == "few_buckets":
        assert all(2 < nz <= 16 for q, nz in holds["ck"])       # (LQ_CK_B)
    else:
        assert all(nz > 16 for q, nz in holds["ck"])
    eng = engine(lib, {"LQCOV_WALK_SHIFT": str(SHIFT)}, monkeypatch)
    try:
        outs = []
        for call in range(3):
            eng.set_profiling(0); eng.set_profiling(2)          # (the stage list starts empty: what is listed ran in this call)
            A = eng.debug_sort_anchors(b["em"], b["off"], b["klib"], n_targets, max_len)
            ran = {s["name"] for s in eng.stage_times() if s["launches"] > 0}
            missing = [s for s in stages if s not in ran]
            assert not missing, "call %d did not reach %s (ran: %s)" % (call, missing, sorted(ran))
            outs.append(A)
    finally:
        eng.close()
    M, off = b["model"], b["off"]
    for call, A in enumerate(outs):
        for q in range(off.shape[0] - 1):
            assert np.array_equal(A[off[q]:off[q + 1]], M[off[q]:off[q + 1]]), "call %d, query %d (%d anchors): %s" % (call, q, off[q + 1] - off[q], first_diff(A, M, off))
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


@pytest.mark.parametrize("name", sorted(GEOM))
def test_emulated_level_with_every_kind_of_sub_array(emu_lib, name, monkeypatch):
    run_case(emu_lib, name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOM))
def test_gpu_level_with_every_kind_of_sub_array(gpu_lib, name, monkeypatch):
    run_case(gpu_lib, name, monkeypatch)

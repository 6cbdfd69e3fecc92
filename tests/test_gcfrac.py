"""The GC fraction step of sampleqc (lq_gcfrac.py:15-55, LqGC.calc_read_and_chunk_gc_frac): a test-local restatement of the
reference's loop, the product (longqc_amd/gcfrac.py over lqgc_reads, kernels_gc.hpp) under the wave emulator and on the GPU
against it -- with the reference's own np.random stream (draw="numpy"), with positions given (the break rule, the short last
slice) and with the device draw, whose documented bijection is restated here in numpy and whose uniformity is tested against
a chi-square quantile."""
import array
import ctypes as C
import itertools
import os
import random
import sys
import types

import numpy as np
import pytest
from scipy.stats import chi2

from longqc_amd import gcfrac as G
from longqc_amd import synth


# ---- restatement of lq_gcfrac.py:15-55 ----
class RefGC:
    """LqGC in the test's words.  draw(l, k) supplies a read's positions (default: np.random.choice, the reference's)."""

    def __init__(self, chunk_size=150, draw=None):
        self.chunk_size = chunk_size
        self.r_frac, self.c_frac = array.array('f'), array.array('f')
        self.r_tot = self.c_tot = self.r_gc_tot = self.c_gc_tot = 0
        self.draw = draw or (lambda l, k: np.random.choice(l, k, replace=False))
        self.dropped = 0                                           # draws the break left unvisited (bookkeeping of the test)

    def calc_read_and_chunk_gc_frac(self, reads, samp_rate=0.2):
        cs = self.chunk_size
        for r in reads:
            s = r[1]
            g, c = ('G', 'C') if isinstance(s, str) else (b'G', b'C')
            l = len(s)
            self.r_tot += l
            gc_n = s.count(g) + s.count(c)
            self.r_frac.append(gc_n / l)
            self.r_gc_tot += gc_n
            indices = self.draw(l, int(float(1 / cs) * l * samp_rate))
            for n_done, i in enumerate(indices):
                i = int(i)
                if i + cs - 1 > l:
                    self.dropped += len(indices) - n_done
                    break
                j = i + cs
                cgc_n = s.count(g, i, j) + s.count(c, i, j)
                self.c_frac.append(float(cgc_n) / cs)
                self.c_gc_tot += cgc_n
                self.c_tot += cs

    def gc_stats(self):
        return [np.mean(self.r_frac), np.std(self.r_frac)]


def assert_same(got, want):
    assert got.r_frac.tobytes() == want.r_frac.tobytes()
    assert got.c_frac.tobytes() == want.c_frac.tobytes()
    assert (got.r_tot, got.c_tot, got.r_gc_tot, got.c_gc_tot) == (want.r_tot, want.c_tot, want.r_gc_tot, want.c_gc_tot)
    assert type(got.r_frac) is array.array and got.r_frac.typecode == 'f' and got.c_frac.typecode == 'f'
    if len(want.r_frac):
        a, b = got.gc_stats(), want.gc_stats()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].dtype == b[0].dtype


def walk(seq: bytes, positions, cs):
    """one read's walk -> (kept, counts of the positions before kept)"""
    l, out = len(seq), []
    for n_done, i in enumerate(positions):
        if i + cs - 1 > l:
            return n_done, out
        out.append(seq.count(b'G', i, i + cs) + seq.count(b'C', i, i + cs))
    return len(positions), out


# ---- restatement of the device draw (kernels_gc.hpp) in numpy ----
M64 = np.uint64(0xffffffffffffffff)


def mix64(z):
    z = (z + np.uint64(0x9e3779b97f4a7c15)) & M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)) & M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)) & M64
    return z ^ (z >> np.uint64(31))


def mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85ebca6b)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xc2b2ae35)
    return x ^ (x >> np.uint32(16))


def ref_draw(seed, first_read, lens, k):
    """positions of all reads, read after read in draw order: the first k[i] images of the bijection of [0, lens[i]) keyed by
    (seed, first_read + i)"""
    lens, k = np.asarray(lens, dtype=np.int64), np.asarray(k, dtype=np.int64)
    with np.errstate(over="ignore"):
        g = np.arange(lens.shape[0], dtype=np.uint64) + np.uint64(first_read)
        a = mix64(mix64(np.full(1, seed, dtype=np.uint64)) ^ g)
        b = mix64(a)
        c = mix64(b)
        rk = [(w >> np.uint64(s)).astype(np.uint32) for w in (a, b, c) for s in (0, 32)]     # (astype keeps the low 32 bits)
        h = np.ones(lens.shape[0], dtype=np.int64)
        for _ in range(16):
            h += (4 ** h < lens)
        rep = lambda v: np.repeat(v, k)
        L_, H_, RK = rep(lens), rep(h).astype(np.uint32), [rep(x) for x in rk]
        m = (np.uint32(1) << H_) - np.uint32(1)
        x = (np.arange(int(k.sum()), dtype=np.int64) - rep(np.cumsum(k) - k)).astype(np.uint32)
        todo = np.ones(x.shape[0], dtype=bool)
        while todo.any():
            Lh, R = x >> H_, x & m
            for r in range(6):
                Lh, R = R, Lh ^ (mix32(R ^ RK[r]) & m)
            y = (Lh << H_) | R
            x = np.where(todo, y, x)
            todo &= x.astype(np.int64) >= L_
    return x


# ---- inputs ----
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def edge_reads(seed):
    """check 2's reads: the edge lengths around chunk_size and 5 * chunk_size (k steps from 0 to 1 at 750), one base, only G,
    lower case and N, a read over several 4096-byte tiles, runs of short reads inside one tile, and reads of 0.8-3 kb whose one
    to four draws are dropped often enough"""
    rng = random.Random(seed)
    seqs = [rand_seq(rng, l) for l in (1, 149, 150, 151, 749, 750, 751)]
    seqs.append("G" * 1000)
    seqs.append(rand_seq(rng, 1200, "ACGTacgtNNS"))
    seqs.append(rand_seq(rng, 21001))
    seqs += [rand_seq(rng, rng.randint(1, 40)) for _ in range(300)]
    seqs += [rand_seq(rng, rng.randint(800, 3000)) for _ in range(150)]
    seqs.append(rand_seq(rng, 9000))
    rng.shuffle(seqs)
    return seqs


def records(seqs, as_bytes):
    return [["r%d" % i, s.encode() if as_bytes else s, "!" * len(s)] for i, s in enumerate(seqs)]


def check_numpy_mode(lib, seed, chunk_size=150, samp_rate=0.2, want_dropped=False):
    seqs = edge_reads(seed)
    cut = [0, 40, 41, 200, len(seqs)]
    chunks = [records(seqs[a:b], as_bytes=(n % 2 == 1)) for n, (a, b) in enumerate(zip(cut, cut[1:]))]
    got, want = G.LqGCMI355X(chunk_size=chunk_size, draw="numpy", lib=lib), RefGC(chunk_size)
    np.random.seed(seed)
    for ch in chunks:
        got.calc_read_and_chunk_gc_frac(ch, samp_rate=samp_rate)
    state = np.random.get_state()[1].copy()
    np.random.seed(seed)
    for ch in chunks:
        want.calc_read_and_chunk_gc_frac(ch, samp_rate=samp_rate)
    assert_same(got, want)
    assert (np.random.get_state()[1] == state).all()               # the generator was consumed as the reference consumes it
    assert len(want.r_frac) == len(seqs)
    if want_dropped:
        assert want.dropped > 0 and len(want.c_frac) > 100          # the seeded inputs hit the break rule
    return want


def check_break_rule(lib):
    rng = random.Random(3)
    for cs, l in ((150, 1000), (150, 151), (64, 200), (1, 5), (4096, 9000)):
        seq = rand_seq(rng, l).encode()
        other = rand_seq(rng, 777).encode()
        base = [p for p in (l - cs, l - cs + 1, l - cs + 2) if 0 <= p < l]
        for perm in itertools.permutations(base):
            pos = list(perm)
            gc, pos_out, win, kept = G.gc_counts([other, seq, other], cs, k=[0, len(pos), 0], pos_in=pos, lib=lib)
            want_kept, want_counts = walk(seq, pos, cs)
            assert list(pos_out) == pos and list(kept) == [0, want_kept, 0], (cs, l, perm)
            assert list(win[:want_kept]) == want_counts and not win[want_kept:].any(), (cs, l, perm)
            assert int(gc[1]) == seq.count(b"G") + seq.count(b"C")
        if l - cs + 1 < l and l - cs + 1 >= 0:                      # the accepted slice of chunk_size - 1 bases
            p = l - cs + 1
            _, _, win, kept = G.gc_counts([seq], cs, k=[1], pos_in=[p], lib=lib)
            assert kept[0] == 1 and win[0] == seq.count(b"G", p) + seq.count(b"C", p)


def check_device_draw(lib, monkeypatch):
    seqs = edge_reads(11)
    lens = np.array([len(s) for s in seqs])
    k = G.draws_per_read(lens, 150, 0.2)
    k[lens == 21001] = 21001                                       # one read drawn in full: the bijection's whole image
    for seed, first in ((0, 0), (12345, 7), (2 ** 64 - 1, 2 ** 40)):
        gc, pos, win, kept = G.gc_counts(seqs, 150, k=k, seed=seed, first_read=first, lib=lib)
        assert (pos == ref_draw(seed, first, lens, k)).all()
        off = np.concatenate([[0], np.cumsum(k)])
        for i, s in enumerate(seqs):
            p = pos[off[i]:off[i + 1]]
            assert (p < len(s)).all() and np.unique(p).shape[0] == p.shape[0]
            want_kept, want_counts = walk(s.encode(), [int(x) for x in p], 150)
            assert kept[i] == want_kept and list(win[off[i]:off[i] + want_kept]) == want_counts and not win[off[i] + want_kept:off[i + 1]].any()
        assert sorted(pos[off[list(lens).index(21001)]:][:21001]) == list(range(21001))
        # the same counts from the positions handed back in
        again = G.gc_counts(seqs, 150, k=k, pos_in=pos, lib=lib)
        assert (again[0] == gc).all() and (again[2] == win).all() and (again[3] == kept).all()
    # the class: one chunk, several chunks and small spans give the same object, and it is the restatement's given the positions
    k = G.draws_per_read(lens, 150, 0.2)
    pos = ref_draw(99, 0, lens, k)
    it = iter(np.split(pos, np.cumsum(k)[:-1]))
    want = RefGC(150, draw=lambda l, kk: next(it))
    want.calc_read_and_chunk_gc_frac(records(seqs, False))
    one = G.LqGCMI355X(draw="device", seed=99, lib=lib)
    one.calc_read_and_chunk_gc_frac(records(seqs, False))
    assert_same(one, want)
    assert (one.last_pos == pos).all() and want.dropped > 0
    monkeypatch.setenv("LQGC_BATCH_BASES", "8192")
    many = G.LqGCMI355X(draw="device", seed=99, lib=lib)
    for a, b in ((0, 1), (1, 100), (100, 101), (101, len(seqs))):
        many.calc_read_and_chunk_gc_frac(records(seqs[a:b], a == 1))
    monkeypatch.delenv("LQGC_BATCH_BASES")
    assert_same(many, want)
    other = G.LqGCMI355X(draw="device", seed=100, lib=lib)
    other.calc_read_and_chunk_gc_frac(records(seqs, False))
    assert other.c_frac.tobytes() != want.c_frac.tobytes() and other.r_frac.tobytes() == want.r_frac.tobytes()


def chi_square(pos, l, bins):
    """Pearson's statistic of positions over `bins` equal parts of [0, l), the expectation from the integers in each part"""
    size = np.bincount(np.arange(l) * bins // l, minlength=bins).astype(np.float64)
    seen = np.bincount(np.asarray(pos, dtype=np.int64) * bins // l, minlength=bins).astype(np.float64)
    exp = size / l * len(pos)
    return float(((seen - exp) ** 2 / exp).sum())


UNIFORM_CASES = ((4096, 5, 3000), (4097, 5, 3000), (800, 1, 12000), (1500, 2, 6000))    # (length, draws per read, reads)


def check_uniformity(lib):
    bins = 16
    bound = chi2.ppf(1 - 1e-6, bins - 1)
    for l, k, n in UNIFORM_CASES:
        assert int(G.draws_per_read(np.array([l]), 150, 0.2)[0]) == k
        seq = b"A" * l
        for seed in (1, 2, 3):
            _, pos, _, _ = G.gc_counts([seq] * n, 150, k=[k] * n, seed=seed, lib=lib)
            stat = chi_square(pos, l, bins)
            print("device draw l=%d k=%d reads=%d seed=%d chi2=%.2f bound=%.2f" % (l, k, n, seed, stat, bound))
            assert stat < bound, (l, k, seed, stat)
            for j in range(k):                                      # and every draw index on its own
                assert chi_square(pos[j::k], l, bins) < bound, (l, k, seed, j)


def raw_call(lib, n, seq, off, cs, k=None, doff=None, pos_in=None, gc=True, win=True, kept=True):
    lib = G._lib(lib)
    arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)
    off, k, doff, pos_in = arr(off, np.uint64), arr(k, np.uint32), arr(doff, np.uint64), arr(pos_in, np.uint32)
    o_gc, o_win, o_kept = np.zeros(n + 1, np.uint32), np.zeros(64, np.uint16), np.zeros(n + 1, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data
    err = C.create_string_buffer(512)
    rc = lib.lqgc_reads(0, n, seq, p(off), cs, p(k), p(doff), p(pos_in), 0, 0, p(o_gc) if gc else None, None,
                        p(o_win) if win else None, p(o_kept) if kept else None, err, 512)
    return rc, err.value.decode(), o_gc


def check_arguments(lib):
    seq = b"ACGT" * 100
    rc, msg, gc = raw_call(lib, 1, seq, [0, 400], 150, [1], [0, 1], [5])
    assert rc == 0 and gc[0] == 200
    assert raw_call(lib, 0, None, [0], 150)[0] == 0                 # n == 0
    assert raw_call(lib, 0, None, [0], 150, [], [0])[0] == 0
    assert G.gc_counts([], lib=lib)[0].shape == (0,)
    for bad in (raw_call(lib, 1, seq, None, 150), raw_call(lib, 1, None, [0, 400], 150), raw_call(lib, 1, seq, [0, 400], 150, gc=False),
                raw_call(lib, 1, seq, [0, 400], 150, [1], None), raw_call(lib, 1, seq, [0, 400], 150, [1], [0, 1], [5], kept=False),
                raw_call(lib, 1, seq, [0, 400], 150, [1], [0, 1], [5], win=False),
                raw_call(lib, 2, seq, [0, 400, 300], 150),          # descending offsets
                raw_call(lib, 1, seq, [0, 400], 150, [401], [0, 401]),    # k[i] > l
                raw_call(lib, 1, seq, [0, 400], 150, [1], [0, 2]),        # draw_off is not k's prefix sum
                raw_call(lib, 1, seq, [0, 400], 150, [1], [0, 1], [400])):    # a position outside the read
        assert bad[0] == -1 and bad[1], bad[:2]
    for cs in (0, 4097):
        rc, msg, _ = raw_call(lib, 1, seq, [0, 400], cs)
        assert rc == -5 and "chunk_size" in msg
    rc, msg, _ = raw_call(lib, 1, seq, [0, 2 ** 32], 150)
    assert rc == -5 and msg
    _, pos, _, kept = G.gc_counts([seq], 1, k=[400], lib=lib)
    assert sorted(pos) == list(range(400)) and kept[0] == 400
    with pytest.raises(G.api.LqcovError):
        G.gc_counts([seq], 0, lib=lib)


def check_exceptions(lib):
    """the two ways the reference's loop raises, and what it leaves behind"""
    rng = random.Random(8)
    seqs = [rand_seq(rng, 900), rand_seq(rng, 1200), "", rand_seq(rng, 700)]
    for draw in ("numpy", "device"):
        got, want = G.LqGCMI355X(draw=draw, seed=4, lib=lib), RefGC()
        np.random.seed(1)
        with pytest.raises(ZeroDivisionError):
            got.calc_read_and_chunk_gc_frac(records(seqs, False))
        if draw == "device":
            it = iter(np.split(got.last_pos, [int(G.draws_per_read(np.array([900]), 150, 0.2)[0])]))
            want.draw = lambda l, k: next(it)
        np.random.seed(1)
        with pytest.raises(ZeroDivisionError):
            want.calc_read_and_chunk_gc_frac(records(seqs, False))
        assert_same(got, want)
        assert len(got.r_frac) == 2
        # samp_rate 200 at chunk_size 150: more draws than bases in the first read already
        got, want = G.LqGCMI355X(draw=draw, lib=lib), RefGC()
        with pytest.raises(ValueError):
            got.calc_read_and_chunk_gc_frac(records(seqs, False), samp_rate=200)
        with pytest.raises(ValueError):
            want.calc_read_and_chunk_gc_frac(records(seqs, False), samp_rate=200)
        assert_same(got, want)
        assert len(got.r_frac) == 1 and got.r_tot == 900 and got.c_tot == 0


# ---- no library needed ----
def test_draws_per_read_equals_the_python_expression():
    for cs, sr in ((150, 0.2), (1, 1.0), (64, 1.0), (4096, 0.2), (150, 0), (150, 1), (7, 0.35), (3, 0.3)):
        lens = np.arange(0, 200000)
        got = G.draws_per_read(lens, cs, sr)
        assert got.tolist() == [int(float(1 / cs) * l * sr) for l in range(200000)], (cs, sr)
    big = np.array([2 ** 32 - 1, 2 ** 31 + 12345, 10 ** 9 + 7])
    assert G.draws_per_read(big, 150, 0.2).tolist() == [int(float(1 / 150) * int(l) * 0.2) for l in big]


def test_the_restated_draw_is_a_bijection():
    for l in (1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000, 4096, 4097, 70000):
        p = ref_draw(5, 9, [l], [l])
        assert sorted(p.tolist()) == list(range(l))
    a = ref_draw(5, 0, [1000, 1000, 1000], [10, 10, 10])
    assert (a[:10] != a[10:20]).any() and (ref_draw(5, 1, [1000, 1000], [10, 10]) == a[10:]).all()     # keyed by the ordinal
    assert (ref_draw(6, 0, [1000], [10]) != a[:10]).any()


def test_numpy_choice_passes_the_uniformity_bound():
    """the same statistic and bound on the reference's own draw: if np.random.choice failed it the bins would be wrong"""
    bins = 16
    bound = chi2.ppf(1 - 1e-6, bins - 1)
    for l, k, n in UNIFORM_CASES:
        for seed in (1, 2, 3):
            np.random.seed(seed)
            pos = np.concatenate([np.random.choice(l, k, replace=False) for _ in range(n)])
            stat = chi_square(pos, l, bins)
            print("np.random.choice l=%d k=%d reads=%d seed=%d chi2=%.2f bound=%.2f" % (l, k, n, seed, stat, bound))
            assert stat < bound
            for j in range(k):
                assert chi_square(pos[j::k], l, bins) < bound
    assert chi_square(np.arange(3000) % 1000, 4096, bins) > bound   # and the statistic does see a draw that is not uniform


def test_restatement_equals_the_reference_class_where_it_imports(monkeypatch):
    ref_dir = os.environ.get("LONGQC_REFERENCE", "/root/reference")   # (the checkout oracle/Makefile builds oracle/_ref from)
    if not os.path.exists(os.path.join(ref_dir, "lq_gcfrac.py")):
        pytest.skip("no reference checkout here")
    m = types.ModuleType("lq_utils")                               # (imports pysam; this step calls nothing of it)
    m.guess_format = m.open_seq_chunk = m.open_seq = None
    monkeypatch.setitem(sys.modules, "lq_utils", m)
    monkeypatch.syspath_prepend(ref_dir)
    monkeypatch.delitem(sys.modules, "lq_gcfrac", raising=False)
    try:
        import lq_gcfrac
    except Exception as e:
        pytest.skip("the reference module does not import: %r" % (e,))
    monkeypatch.delitem(sys.modules, "lq_gcfrac", raising=False)
    seqs = edge_reads(4)
    a, b = lq_gcfrac.LqGC(chunk_size=150), RefGC(150)
    np.random.seed(7)
    a.calc_read_and_chunk_gc_frac(records(seqs, False))
    np.random.seed(7)
    b.calc_read_and_chunk_gc_frac(records(seqs, False))
    assert a.r_frac == b.r_frac and a.c_frac == b.c_frac
    assert (a.r_tot, a.c_tot, a.r_gc_tot, a.c_gc_tot) == (b.r_tot, b.c_tot, b.r_gc_tot, b.c_gc_tot)


# ---- the emulator build ----
def test_emulated_numpy_draw_equals_the_restatement(emu_lib):
    check_numpy_mode(emu_lib, seed=1, want_dropped=True)


def test_emulated_numpy_draw_in_small_spans(emu_lib, monkeypatch):
    monkeypatch.setenv("LQGC_BATCH_BASES", "4096")                  # the 21-kb read and many others lie over span boundaries
    check_numpy_mode(emu_lib, seed=2, want_dropped=True)


@pytest.mark.parametrize("chunk_size,samp_rate", [(1, 0.2), (1, 1.0), (64, 1.0), (4096, 1.0), (150, 0), (150, 1.0), (150, 1)])
def test_emulated_other_chunk_sizes_and_rates(emu_lib, chunk_size, samp_rate):
    check_numpy_mode(emu_lib, seed=3 + chunk_size, chunk_size=chunk_size, samp_rate=samp_rate)


def test_emulated_break_rule_and_short_last_slice(emu_lib):
    check_break_rule(emu_lib)


def test_emulated_device_draw(emu_lib, monkeypatch):
    check_device_draw(emu_lib, monkeypatch)


def test_emulated_device_draw_is_uniform(emu_lib):
    check_uniformity(emu_lib)


def test_emulated_arguments(emu_lib):
    check_arguments(emu_lib)


def test_emulated_exceptions(emu_lib):
    check_exceptions(emu_lib)


# ---- the gfx950 build ----
@pytest.mark.gpu
def test_gpu_numpy_draw_equals_the_restatement(gpu_lib, monkeypatch):
    check_numpy_mode(gpu_lib, seed=1, want_dropped=True)
    monkeypatch.setenv("LQGC_BATCH_BASES", "4096")
    check_numpy_mode(gpu_lib, seed=2, want_dropped=True)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_size,samp_rate", [(1, 0.2), (1, 1.0), (64, 1.0), (4096, 1.0), (150, 0), (150, 1.0), (150, 1)])
def test_gpu_other_chunk_sizes_and_rates(gpu_lib, chunk_size, samp_rate):
    check_numpy_mode(gpu_lib, seed=3 + chunk_size, chunk_size=chunk_size, samp_rate=samp_rate)


@pytest.mark.gpu
def test_gpu_break_rule_and_short_last_slice(gpu_lib):
    check_break_rule(gpu_lib)


@pytest.mark.gpu
def test_gpu_device_draw(gpu_lib, monkeypatch):
    check_device_draw(gpu_lib, monkeypatch)


@pytest.mark.gpu
def test_gpu_device_draw_is_uniform(gpu_lib):
    check_uniformity(gpu_lib)


@pytest.mark.gpu
def test_gpu_arguments_and_exceptions(gpu_lib):
    check_arguments(gpu_lib)
    check_exceptions(gpu_lib)


@pytest.mark.gpu
def test_gpu_chunk_of_50k_reads_both_draws(gpu_lib):
    """configs[1]'s 50 000 reads (~750 Mbases) as one chunk: draw="numpy" equals the restatement in full, draw="device" equals
    it given the positions the device drew, which are the restated bijection's"""
    fr = synth.make_reads_flat(synth.CONFIGS["cfg2"], workers=16)
    flat = fr.flat.tobytes()
    recs = [["r%d" % i, flat[int(fr.off[i]):int(fr.off[i + 1])]] for i in range(len(fr))]
    assert len(recs) == 50000
    got, want = G.LqGCMI355X(draw="numpy", lib=gpu_lib), RefGC()
    np.random.seed(50)
    got.calc_read_and_chunk_gc_frac(recs)
    np.random.seed(50)
    want.calc_read_and_chunk_gc_frac(recs)
    assert_same(got, want)
    assert want.dropped > 0 and len(want.c_frac) > 500000
    dev = G.LqGCMI355X(draw="device", seed=50, lib=gpu_lib)
    dev.calc_read_and_chunk_gc_frac(recs)
    lens = np.diff(fr.off.astype(np.int64))
    k = G.draws_per_read(lens, 150, 0.2)
    assert (dev.last_pos == ref_draw(50, 0, lens, k)).all()
    it = iter(np.split(dev.last_pos, np.cumsum(k)[:-1]))
    given = RefGC(150, draw=lambda l, kk: next(it))
    given.calc_read_and_chunk_gc_frac(recs)
    assert_same(dev, given)
    assert dev.r_frac.tobytes() == want.r_frac.tobytes()

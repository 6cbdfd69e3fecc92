"""The adapter search of sampleqc (lq_adapt.py:10-101): a test-local restatement of what edlib.align(adapter, window,
mode="HW", task="path") reports (explicit matrices and traceback), checked against edlib itself where it can be imported, the
product's kernel (kernels_adapt.hpp) under the wave emulator and on the GPU against the restatement, and
longqc_amd.adapter.cut_adapter against a restatement of lq_adapt.cut_adapter built on the restated align."""
import array
import ctypes as C
import dataclasses
import random
import re

import numpy as np
import pytest

from longqc_amd import adapter as A
from longqc_amd import sampleqc, synth


# ---- restatement of edlib's HW alignment (edlib.cpp: HW end search, reverse SHW start search, NW traceback) ----
def edlib_hw(adp, win):
    """-> (d, (s, e), L, ops): the edit distance, locations[0], the length of the alignment path and its ops (= match, X
    mismatch, I adapter base against a gap, D window base against a gap)"""
    m, n = len(adp), len(win)
    prev = [0] * (n + 1)                                       # HW: row 0 free
    for i in range(1, m + 1):
        cur = [i] + [0] * n
        a = adp[i - 1]
        for j in range(1, n + 1):
            cur[j] = min(prev[j - 1] + (a != win[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    d = min(prev)
    e = prev.index(d) - 1                                      # first end; column 0 is end -1
    if e < 0:
        return d, (0, e), m, "I" * m
    # start: the smallest s with NW(adp, win[s..e]) == d (edlib's reverse pass keeps the longest alignment)
    R = [[0] * (e + 2) for _ in range(m + 1)]
    for j in range(e + 1, -1, -1):
        R[m][j] = e + 1 - j
    for i in range(m - 1, -1, -1):
        R[i][e + 1] = m - i
        for j in range(e, -1, -1):
            R[i][j] = min(R[i + 1][j + 1] + (adp[i] != win[j]), R[i + 1][j] + 1, R[i][j + 1] + 1)
    s = next(j for j in range(e + 1) if R[0][j] == d)
    # NW matrix of adp x win[s..e] and edlib's traceback: up if up + 1 == score, else left if left + 1 == score, else diagonal
    t = win[s:e + 1]
    W = len(t)
    D = [[0] * (W + 1) for _ in range(m + 1)]
    for j in range(W + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        D[i][0] = i
        for j in range(1, W + 1):
            D[i][j] = min(D[i - 1][j - 1] + (adp[i - 1] != t[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    assert D[m][W] == d
    i, j, ops = m, W, []
    while i > 0 or j > 0:
        if i > 0 and D[i - 1][j] + 1 == D[i][j]:
            ops.append("I"); i -= 1
        elif j > 0 and D[i][j - 1] + 1 == D[i][j]:
            ops.append("D"); j -= 1
        else:
            ops.append("=" if adp[i - 1] == t[j - 1] else "X"); i -= 1; j -= 1
    ops = "".join(reversed(ops))
    return d, (s, e), len(ops), ops


def _cigar(ops):
    return "".join("%d%s" % (len(g.group(0)), g.group(0)[0]) for g in re.finditer(r"(.)\1*", ops))


def align(adp, win, mode="HW", task="path"):
    """the restated edlib.align, the fields lq_adapt.py reads"""
    d, loc, _, ops = edlib_hw(adp, win)
    return {"editDistance": d, "locations": [loc], "cigar": _cigar(ops)}


# ---- restatement of lq_adapt.py on the restated align (lq_adapt.py:10-101, its statements in its order) ----
_REPAT = re.compile(r'(\d+)[DHIMNPSX=]{1}')


def _ref_cut(reads, adp, th, r, three, len_list=[], align=align):
    iden_max, match_num, cut_pos, skip_num = -1, 0, [], 0
    has_qual = len(reads[0]) > 2
    for read in reads:
        read_length = len(read[1])
        if len_list:
            len_list.append(read_length)
        if read_length < 2 * r:
            skip_num += 1
            continue
        result = align(adp, read[1][-r:] if three else read[1][:r])
        identity = 1.0 - float(result['editDistance'] / np.sum([int(i) for i in _REPAT.findall(result['cigar'])]))
        if identity > th:
            if three:
                start = len(read[1]) - r + result['locations'][0][0]
                cut_pos.append(r - result['locations'][0][0])
            else:
                end = result['locations'][0][1]
                cut_pos.append(end)
            match_num += 1
            if identity > iden_max:
                iden_max = identity
            if three:
                read[1] = read[1][:start]
                if has_qual:
                    read[2] = read[2][:start]
            else:
                read[1] = read[1][end + 1:]
                if has_qual:
                    read[2] = read[2][end + 1:]
    return (iden_max, match_num, cut_pos)


def ref_cut_adapter(reads, len_list=None, adp_t=None, adp_b=None, th=0.75, length=150, align=align):
    if not adp_t and not adp_b:
        return None
    if adp_t and adp_b:
        return (_ref_cut(reads, adp_t, th, length, False, len_list=len_list, align=align),
                _ref_cut(reads, adp_b, th, length, True, align=align))
    if adp_t:
        return _ref_cut(reads, adp_t, th, length, False, len_list=len_list, align=align)
    return _ref_cut(reads, adp_b, th, length, True, len_list=len_list, align=align)


# ---- inputs ----
def mutate(s, rng, err):
    out = []
    for ch in s:
        x = rng.random()
        if x < err / 3:
            out.append(rng.choice("ACGT"))                     # substitution (possibly to itself)
        elif x < 2 * err / 3:
            out.append(ch + rng.choice("ACGT"))                # insertion after
        elif x >= err:
            out.append(ch)                                     # (else: deletion)
    return "".join(out)


def rand_seq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def implant(seq, adp, rng, err, where, at):
    """the adapter, mutated at `err`, written over seq from `at` bases off the read's 5' (where=5) or 3' end"""
    a = mutate(adp, rng, err)
    if where == 5:
        return seq[:at] + a + seq[at + len(a):]
    k = len(seq) - at - len(a)
    return seq[:k] + a + seq[k + len(a):]


def mixed_reads(rng, n, adp5, adp3, length=150):
    """random reads, implanted adapters with substitutions and indels, tandem windows, N and lower case, edge lengths"""
    reads = []
    for i in range(n):
        kind = i % 8
        ln = rng.choice([0, 2 * length - 1, 2 * length, 2 * length + 1, rng.randint(2 * length, 5 * length), rng.randint(0, 4 * length)])
        if kind == 0:
            s = rand_seq(rng, ln)
        elif kind == 1:
            unit = rand_seq(rng, rng.randint(1, 6))
            s = (unit * (ln // max(1, len(unit)) + 1))[:ln]
            s = mutate(s, rng, 0.03)
        elif kind == 2:
            s = rand_seq(rng, ln, "ACGTNacgt")
        else:
            s = rand_seq(rng, ln)
            if len(s) >= 2 * length:
                if adp5:
                    s = implant(s, adp5, rng, rng.choice([0.0, 0.05, 0.12, 0.3]), 5, rng.randint(0, 40))
                if adp3:
                    s = implant(s, adp3, rng, rng.choice([0.0, 0.05, 0.12, 0.3]), 3, rng.randint(0, 40))
        reads.append(s)
    return reads


def hits_want(seqs, adp, length, which):
    out = np.full((len(seqs), 4), -1, dtype=np.int32)
    for i, s in enumerate(seqs):
        if len(s) >= 2 * length:
            d, (st, e), L, _ = edlib_hw(adp, s[:length] if which == 5 else s[-length:])
            out[i] = (d, st, e, L)
    return out


# ---- CPU: the restatement ----
TABLE = [("ACGT", "TTACGTTT", (0, (2, 5), 4, "====")),
         ("ACGTACGT", "GGACGTTACGTGG", (1, (2, 10), 9, "====D====")),
         ("AACC", "GGACACGG", (2, (1, 3), 4, "X==I")),
         ("CAT", "GGCTAGG", (1, (2, 3), 3, "=I="))]


@pytest.mark.parametrize("adp,win,want", TABLE)
def test_restatement_gives_the_issue_table(adp, win, want):
    assert edlib_hw(adp, win) == want


def test_restatement_ties_and_edges():
    assert edlib_hw("AB", "BA")[2] in (2, 3)
    assert edlib_hw("AAA", "") == (3, (0, -1), 3, "III")
    assert edlib_hw("AC", "GGGG") == (2, (0, -1), 2, "II")
    d, (s, e), L, ops = edlib_hw("ACGT", "ACGTACGT")                 # two exact ends: the first
    assert (d, s, e) == (0, 0, 3)


def test_restatement_equals_edlib():
    edlib = pytest.importorskip("edlib")
    rng = random.Random(11)
    n = 0
    for _ in range(3000):
        m = rng.choice([1, 2, 3, 5, 8, 18, 30, 64, 65])
        w = rng.randint(1, 160)
        alpha = rng.choice(["ACGT", "AC", "A", "ACGTN"])
        adp = rand_seq(rng, m, alpha)
        win = rand_seq(rng, w, alpha) if rng.random() < 0.5 else implant(rand_seq(rng, max(w, m + 2), alpha), adp, rng, 0.15, 5, rng.randint(0, 5))
        r = edlib.align(adp, win, mode="HW", task="path")
        d, loc, L, _ = edlib_hw(adp, win)
        assert r["editDistance"] == d, (adp, win)
        assert tuple(r["locations"][0]) == loc, (adp, win)
        assert sum(int(i) for i in _REPAT.findall(r["cigar"])) == L, (adp, win)
        n += 1
    assert n == 3000


# ---- the C entry point and cut_adapter, on a library (emulator or GPU build) ----
def call_reads(lib, seqs, adp5, adp3, length):
    raw = [s.encode() for s in seqs]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in raw])
    flat = b"".join(raw)
    o5 = np.zeros((max(len(raw), 1), 4), np.int32)
    o3 = np.zeros((max(len(raw), 1), 4), np.int32)
    err = C.create_string_buffer(512)
    A._lib(lib)
    rc = lib.lqadapt_reads(0, len(raw), flat or None, off.ctypes.data, adp5.encode() if adp5 else None, len(adp5) if adp5 else 0,
                           adp3.encode() if adp3 else None, len(adp3) if adp3 else 0, length, o5.ctypes.data, o3.ctypes.data, err, 512)
    return rc, o5[:len(raw)], o3[:len(raw)], err.value.decode()


def check_c_entry_point(lib, adapter_lens, n_reads, seed, length=150):
    rng = random.Random(seed)
    for m in adapter_lens:
        adp5, adp3 = rand_seq(rng, m), rand_seq(rng, m + 1 if m > 1 else 1)
        seqs = mixed_reads(rng, n_reads, adp5, adp3, length)
        rc, o5, o3, err = call_reads(lib, seqs, adp5, adp3, length)
        assert rc == 0, err
        np.testing.assert_array_equal(o5, hits_want(seqs, adp5, length, 5), err_msg="5' m=%d" % m)
        np.testing.assert_array_equal(o3, hits_want(seqs, adp3, length, 3), err_msg="3' m=%d" % (m + 1))


def check_arguments(lib):
    rc, o5, o3, _ = call_reads(lib, ["ACGT" * 100], "ACGT", None, 150)
    assert rc == 0 and (o5[0] == (0, 0, 3, 4)).all() and (o3 == 0).all()       # 3' not asked for: out3 untouched
    assert call_reads(lib, [], "ACGT", "ACGT", 150)[0] == 0
    assert call_reads(lib, ["A" * 400], "ACGT", None, 0)[0] == -5
    assert call_reads(lib, ["A" * 400], "ACGT", None, 4097)[0] == -5
    with pytest.raises(Exception):
        A.adapter_hits(["A" * 400], "ACGT", 0, lib=lib)


def fresh(reads):
    return [list(r) for r in reads]


def check_cut_adapter(lib, seed, n_reads=60, length=150):
    rng = random.Random(seed)
    adp5, adp3 = sampleqc.PRESET_ADAPTERS["pb-sequel"][0], sampleqc.PRESET_ADAPTERS["ont-ligation"][1]
    seqs = mixed_reads(rng, n_reads, adp5, adp3, length)
    # reads that the 5' trim takes below 2 * length: the 3' pass must skip them
    for k in range(3):
        s = rand_seq(rng, 2 * length + k)
        seqs.append(implant(implant(s, adp5, rng, 0.0, 5, 60), adp3, rng, 0.0, 3, 0))
    recs = [["r%d" % i, s, "".join(chr(33 + rng.randint(0, 40)) for _ in s)] for i, s in enumerate(seqs)]
    for kw in (dict(adp_t=adp5, adp_b=adp3), dict(adp_t=adp5), dict(adp_b=adp3), dict(adp_t=adp5, adp_b=adp3, th=0.6)):
        for ll in (None, [], [7]):
            a, b = fresh(recs), fresh(recs)
            la, lb = (list(ll) if ll is not None else None), (list(ll) if ll is not None else None)
            got = A.cut_adapter(a, len_list=la, length=length, lib=lib, **kw)
            want = ref_cut_adapter(b, len_list=lb, length=length, **kw)
            assert got == want, kw
            assert a == b and la == lb, kw
    two = A.cut_adapter(fresh(recs), adp_t=adp5, adp_b=adp3, length=length, lib=lib)
    assert two[0][1] > 0 and two[1][1] > 0                                         # the implants are found
    # records without qualities (fewer than three fields): only seq is cut
    a2 = [[r[0], r[1]] for r in recs]
    b2 = [[r[0], r[1]] for r in recs]
    assert A.cut_adapter(a2, adp_t=adp5, adp_b=adp3, length=length, lib=lib) == ref_cut_adapter(b2, adp_t=adp5, adp_b=adp3, length=length)
    assert a2 == b2
    assert A.cut_adapter(fresh(recs), lib=lib) is None
    # LongQC's pool trims a pickled copy: a shallow copy of every record leaves the chunk as it was
    before = [list(r) for r in recs]
    A.cut_adapter([list(r) for r in recs], adp_t=adp5, adp_b=adp3, length=length, lib=lib)
    assert recs == before


def test_cut_adapter_skip_after_5p_trim_is_restated():
    """the 3' skip sees the 5'-trimmed length (lq_adapt.py:95-96 run _cutr on what _cutf left)"""
    adp = "ACGTTGCAACGGTTAC"
    s = adp + "T" * (300 - len(adp))
    recs = [["r", s, "!" * len(s)]]
    t5, t3 = ref_cut_adapter(recs, adp_t=adp, adp_b="GGGGGGGGGG", length=150)
    assert t5[1] == 1 and len(recs[0][1]) < 300 and t3 == (-1, 0, [])


@pytest.mark.parametrize("m", [1, 18, 45, 63, 64, 65, 130])
def test_emulated_adapt_reads_equal_the_restatement(emu_lib, m):
    check_c_entry_point(emu_lib, [m], 24, seed=100 + m)


@pytest.mark.parametrize("length,m", [(20, 45), (1, 18), (1000, 130), (333, 64)])
def test_emulated_adapt_reads_other_window_lengths(emu_lib, length, m):
    """windows shorter than the adapter, of one base, and long windows through the banded (m > 64) and one-band forms"""
    check_c_entry_point(emu_lib, [m], 24 if length < 300 else 8, seed=length + m, length=length)


def test_emulated_adapt_reads_in_small_batches(emu_lib, monkeypatch):
    monkeypatch.setenv("LQADAPT_BATCH_READS", "7")                  # several uploads / launches per adapter
    check_c_entry_point(emu_lib, [45], 50, seed=5)
    check_c_entry_point(emu_lib, [70], 20, seed=6)


def test_emulated_adapt_arguments(emu_lib):
    check_arguments(emu_lib)


def test_emulated_cut_adapter_equals_the_restated_reference(emu_lib):
    check_cut_adapter(emu_lib, seed=21)


def test_adapter_stats_mirror_longqc():
    st = A.AdapterStats("ACGT", "TTTT")
    st.add(((0.8, 2, [10, 20]), (-1, 0, [])))
    st.add(((0.9, 1, [30]), (0.7, 1, [5])))
    blk = st.json_block()
    assert blk == {"Stats_for_adapter5": {"Num_of_trimmed_reads_5": 3, "Max_identity_adp5": 0.9, "Average_position_from_5_end": 20.0}}
    assert A.AdapterStats(adp3="TTTT").json_block() == {}
    only3 = A.AdapterStats(adp3="TTTT")
    only3.add((0.75, 1, [7]))
    assert only3.json_block() == {"Stats_for_adapter3": {"Num_of_trimmed_reads_3": 1, "Max_identity_adp3": 0.75,
                                                         "Average_position_from_3_end": np.mean(array.array('i', [7]))}}


def test_preset_adapters_cover_every_preset():
    assert set(sampleqc.PRESET_ADAPTERS) == set(sampleqc.PRESET_MED_SCORE)
    assert len(sampleqc.PRESET_ADAPTERS["ont-1dsq"][1]) == 64 and sampleqc.PRESET_ADAPTERS["ont-rapid"][1] is None


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 18, 45, 63, 64, 65, 130])
def test_gpu_adapt_reads_equal_the_restatement(gpu_lib, m):
    check_c_entry_point(gpu_lib, [m], 60, seed=300 + m)


@pytest.mark.gpu
@pytest.mark.parametrize("length,m", [(20, 45), (1, 18), (1000, 130), (4096, 65)])
def test_gpu_adapt_reads_other_window_lengths(gpu_lib, length, m):
    check_c_entry_point(gpu_lib, [m], 40 if length < 300 else 6, seed=length + m, length=length)


@pytest.mark.gpu
def test_gpu_adapt_reads_in_small_batches_and_arguments(gpu_lib, monkeypatch):
    check_arguments(gpu_lib)
    monkeypatch.setenv("LQADAPT_BATCH_READS", "7")
    check_c_entry_point(gpu_lib, [45, 70], 40, seed=8)


@pytest.mark.gpu
def test_gpu_cut_adapter_equals_the_restated_reference(gpu_lib):
    check_cut_adapter(gpu_lib, seed=22)


@pytest.mark.gpu
def test_gpu_empty_chunk_and_no_adapter(gpu_lib):
    assert A.cut_adapter([], adp_t="ACGT", adp_b="TTGA", lib=gpu_lib) == ((-1, 0, []), (-1, 0, []))
    assert A.cut_adapter([], adp_t="ACGT", lib=gpu_lib) == (-1, 0, [])
    assert A.adapter_hits([], "ACGT", lib=gpu_lib).shape == (0, 4)
    assert A.cut_adapter([["r", "ACGT" * 100, "!" * 400]], lib=gpu_lib) is None


def chunk_reads(n, seed, adp5, adp3):
    """n synthetic reads (synth.py, configs[2]'s error model, 100 to ~6 kb) with adapters implanted at the read ends of
    about a third of them at 0-15 % error, 0-20 bases in"""
    cfg = dataclasses.replace(synth.CONFIGS["cfg3"], name="adp", n_reads=n, mean_len=1500, min_len=100, seed=seed)
    fr = synth.make_reads_flat(cfg)
    flat = fr.flat.tobytes().decode("latin-1")
    rng = np.random.default_rng(seed)
    prng = random.Random(seed)
    seqs = []
    for i in range(n):
        s = flat[int(fr.off[i]):int(fr.off[i + 1])]
        if len(s) >= 300:
            if adp5 and rng.random() < 0.35:
                s = implant(s, adp5, prng, float(rng.choice([0.0, 0.05, 0.15])), 5, int(rng.integers(0, 20)))
            if adp3 and rng.random() < 0.35:
                s = implant(s, adp3, prng, float(rng.choice([0.0, 0.05, 0.15])), 3, int(rng.integers(0, 20)))
        seqs.append(s)
    return seqs


@pytest.mark.gpu
@pytest.mark.parametrize("preset", sorted(sampleqc.PRESET_ADAPTERS))
def test_gpu_chunk_of_200k_reads_per_preset(gpu_lib, preset):
    adp5, adp3 = sampleqc.PRESET_ADAPTERS[preset]
    seqs = chunk_reads(200000, 5000 + sorted(sampleqc.PRESET_ADAPTERS).index(preset), adp5, adp3)
    o5 = A.adapter_hits(seqs, adp5, 150, 5, lib=gpu_lib)
    o3 = A.adapter_hits(seqs, adp3, 150, 3, lib=gpu_lib) if adp3 else None
    ok = np.array([len(s) >= 300 for s in seqs])
    assert ok.sum() > 150000 and (~ok).sum() > 0
    assert (o5[~ok] == -1).all() and (o5[ok, 0] >= 0).all()
    # every field of a seeded sample of ends against the restatement
    rng = np.random.default_rng(1)
    sample = rng.choice(np.flatnonzero(ok), 250, replace=False)
    for i in sample.tolist():
        for adp, o, which in ((adp5, o5, 5), (adp3, o3, 3)):
            if adp:
                d, (s, e), L, _ = edlib_hw(adp, seqs[i][:150] if which == 5 else seqs[i][-150:])
                assert tuple(o[i]) == (d, s, e, L), (preset, which, i)
    # cut_adapter on the whole chunk equals the restated lq_adapt.cut_adapter whose align() answers with the GPU's per-end
    # results (checked on the sample above): the skips, identities, trims and the 5'-then-3' order at chunk size
    table = {}
    for adp, o, which in ((adp5, o5, 5), (adp3, o3, 3)):
        if adp:
            for i in np.flatnonzero(ok).tolist():
                d, s, e, L = (int(x) for x in o[i])
                table[(adp, seqs[i][:150] if which == 5 else seqs[i][-150:])] = {"editDistance": d, "locations": [(s, e)], "cigar": "%dM" % L}

    def gpu_align(adp, win):
        return table[(adp, win)]                   # (a 3' window the reference aligns is the untrimmed read's: KeyError otherwise)
    recs = [["r%d" % i, s, "!" * len(s)] for i, s in enumerate(seqs)]
    a, b = fresh(recs), fresh(recs)
    la, lb = [0], [0]
    got = A.cut_adapter(a, len_list=la, adp_t=adp5, adp_b=adp3, lib=gpu_lib)
    assert got == ref_cut_adapter(b, len_list=lb, adp_t=adp5, adp_b=adp3, align=gpu_align)
    assert a == b and la == lb
    t5 = got[0] if adp3 else got
    assert t5[1] > 0.25 * ok.sum() and t5[0] == 1.0


@pytest.mark.gpu
def test_gpu_cut_adapter_chunk_equals_the_restated_reference(gpu_lib):
    """a chunk of a few hundred synthetic reads through the whole of cut_adapter, both sides, against lq_adapt restated"""
    adp5, adp3 = sampleqc.PRESET_ADAPTERS["ont-1dsq"]
    seqs = chunk_reads(400, 77, adp5, adp3)
    recs = [["r%d" % i, s, "!" * len(s)] for i, s in enumerate(seqs)]
    a, b = fresh(recs), fresh(recs)
    la, lb = [0], [0]
    assert A.cut_adapter(a, len_list=la, adp_t=adp5, adp_b=adp3, lib=gpu_lib) == ref_cut_adapter(b, len_list=lb, adp_t=adp5, adp_b=adp3)
    assert a == b and la == lb

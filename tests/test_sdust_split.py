"""The low-complexity scan in pieces (kernels_dust_split.hpp): lqchunk_sdust_split and lqchunk_sdust_intervals against the
serial walk (lqchunk_sdust), the golden tables the reference binary wrote and the oracle's lqo_sdust_masked -- under the wave emulator, in
its three thread orders, and on the GPU.  The pieces are made tiny (2 W + 2 bases, the smallest the call takes) so that reads of a few
hundred bases are cut many times; the launch-cap check follows tests/test_launch_caps.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from longqc_amd import chunkpass, sdust
from tests import oracle_bind
from tests.conftest import GOLDEN, ROOT, read_gz
from tests.helpers import read_fastx
from tests.test_launch_caps import ORDERS, assert_past_cap, header_define, set_order
from tests.test_sdust import CASES

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CSRC = os.path.join(ROOT, "longqc_amd", "csrc")


def oracle_masked():
    """lqo_sdust_masked of oracle/liblqcov_oracle.so: the masked bases of one read"""
    so = os.path.join(oracle_bind.ORACLE_DIR, "liblqcov_oracle.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", oracle_bind.ORACLE_DIR, "oracle"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    ora = C.CDLL(so)
    ora.lqo_sdust_masked.restype = C.c_uint32
    ora.lqo_sdust_masked.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
    return lambda seq, w, t: int(ora.lqo_sdust_masked(seq.encode() if isinstance(seq, str) else bytes(seq), len(seq), t, w))


def load(lib, seqs, quals=None):
    reads = [["r%d" % i, s if isinstance(s, str) else bytes(s).decode()] + ([quals[i]] if quals is not None else []) for i, s in enumerate(seqs)]
    return chunkpass.ReadChunk(reads, lib=lib)


def rand_seq(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes().decode()


def test_the_python_constants_are_the_headers():
    assert sdust.SPLIT_MIN_PIECES == header_define("LQ_DUST_SPLIT_MIN_PIECES") and sdust.SPLIT_PIECE == header_define("LQ_DUST_SPLIT_PIECE")


def split_min(piece):
    """LQ_DUST_SPLIT_MIN: the fewest bases of a read that is cut"""
    return sdust.SPLIT_MIN_PIECES * piece


# ---- 1. the golden tables ---------------------------------------------------------------------------------------------------
def golden_inputs():
    """(file, W, T, golden table) of sdust_cases.json"""
    for case in CASES:
        argv, w, t = list(case["argv"]), 64, 20
        while len(argv) > 1:
            a = argv.pop(0)
            v = a[2:] if len(a) > 2 else argv.pop(0)
            w, t = (int(v), t) if a[1] == "w" else (w, int(v))
        yield argv[0], w, t, case["expect"]


def check_golden(lib):
    cut = 0
    for fn, w, t, expect in golden_inputs():
        names, seqs, quals = read_fastx(os.path.join(GOLDEN, fn))
        qs = [bytes(q).decode() for q in quals] if quals is not None else None
        ch = load(lib, seqs, qs)
        want = ch.sdust(w, t)
        for piece in (2 * w + 2, 200, None):
            got = ch.sdust(w, t, split="pieces", piece=piece)
            for g, x, what in zip(got, want, ("masked", "psum", "qv")):
                assert g.tobytes() == x.tobytes(), (fn, w, t, piece, what)
            assert ch.n_serial == sum(1 for s in seqs if len(s) < split_min(piece or sdust.SPLIT_PIECE) or set(bytes(s).upper()) - set(b"ACGT"))
            cut += ch.n - ch.n_serial
            rows = sdust.sdust_rows(names, None, None, w=w, t=t, chunk=ch, split="pieces", piece=piece)
            assert "\n".join(rows) + "\n" == read_gz(expect)
        ch.close()
        rows = sdust.sdust_rows(names, seqs, quals, w=w, t=t, lib=lib, split="pieces", piece=2 * w + 2)      # (a chunk of its own)
        assert "\n".join(rows) + "\n" == read_gz(expect)
    assert cut > 100                                                # the fixtures' reads are cut


# ---- 2. the smallest shapes that can go wrong -------------------------------------------------------------------------------
def edge_reads(w, piece):
    """the issue's list, for pieces of `piece` bases: every read has at least two pieces' bases and no byte but A/C/G/T"""
    rng = np.random.default_rng(1000 + w)
    low = lambda n: "".join("AC"[int(x)] for x in rng.integers(0, 2, n))
    return [
        "A" * 300,
        "AT" * 150,
        ("ACGGTCA" * 58)[:400],
        rand_seq(rng, 2 * w) + "AAT" * 90,                           # random for 2 W bases, then low complexity over many borders
        rand_seq(rng, piece - 7) + "T" * 14 + rand_seq(rng, piece - 7) + low(40) + rand_seq(rng, 2 * piece),          # runs over the first two borders
        # a piece multiple.  Low complexity begins at the second border: its first perfect intervals start in the random piece before it
        (low(piece) + rand_seq(rng, piece) + "GA" * piece)[:3 * piece],
        (low(piece) + rand_seq(rng, piece) + "GA" * piece)[:3 * piece] + "G",                                        # and a base longer
        ("acgtt" * 20 + "a" * 120 + rand_seq(rng, 60).lower() + "TTTTTTTTTg" * 12),                                  # lower case
        rand_seq(rng, 700),
    ]


EDGE_WT = [(w, t) for w in (3, 8, 64, 66) for t in (5, 20)]


def check_edges(lib, wt=EDGE_WT):
    masked_of = oracle_masked()
    total = 0
    for w, t in wt:
        piece = 2 * w + 2
        seqs = edge_reads(w, piece)
        assert all(len(s) >= split_min(piece) for s in seqs)
        assert len(seqs[5]) % piece == 0 and len(seqs[6]) % piece == 1
        want = [masked_of(s, w, t) for s in seqs]
        ch = load(lib, seqs)
        got, _, _ = ch.sdust(w, t, split="pieces", piece=piece)
        assert ch.n_serial == 0
        assert got[:len(seqs)].tolist() == want, (w, t)
        assert ch.sdust(w, t)[0][:len(seqs)].tolist() == want
        ch.close()
        total += sum(want)
        if w >= 64:
            assert want[0] == 300 and want[1] == 300 and 0 < want[3] < len(seqs[3])
    assert total > 1000


# ---- 3. who takes the serial walk -------------------------------------------------------------------------------------------
def check_serial_routing(lib):
    masked_of = oracle_masked()
    w, t, piece = 64, 20, 130
    rng = np.random.default_rng(3)
    unit = "AT" * 40 + "N" + "AT" * 40 + "N" + "AT" * 40
    with_n = unit * (split_min(piece) // len(unit) + 1)
    with_u = "AC" * 100 + "U" + rand_seq(rng, 300)
    short = ("AAG" * 200)[:split_min(piece) - 1]
    cut = ("AAG" * 200)[:split_min(piece)]
    seqs = [with_n, cut, with_u, short, rand_seq(rng, 500)]
    assert len(with_n) >= split_min(piece) and len(with_u) >= split_min(piece)
    ch = load(lib, seqs)
    got, _, _ = ch.sdust(w, t, split="pieces", piece=piece)
    assert ch.n_serial == 3
    assert got[:5].tolist() == [masked_of(s, w, t) for s in seqs]
    assert got[0] > 0 and got[2] > 0 and got[3] > 0
    _, _, flagged = ch.sdust_intervals(w, t, piece)
    assert flagged.tolist() == [True, False, True, False, False]          # (the intervals serve a read of any length)
    ch.close()


def check_errors(lib):
    from longqc_amd import api
    ch = load(lib, ["ACGT" * 100])
    for w, piece, code in ((64, 129, -1), (8, 17, -1), (2, 200, -5), (67, 200, -5)):
        with pytest.raises(api.LqcovError) as e:
            ch.sdust(w, 20, split="pieces", piece=piece)
        assert e.value.code == code, (w, piece, e.value)
    with pytest.raises(ValueError):
        ch.sdust(64, 20, split="halves")
    assert ch.sdust(64, 20, split="pieces", piece=130)[0][0] == ch.sdust(64, 20, split="serial")[0][0]
    for piece in (-1, 1 << 32):                                     # (what does not fit the call's 32 bits is refused, not wrapped)
        with pytest.raises(ValueError):
            ch.sdust(64, 20, split="pieces", piece=piece)
        with pytest.raises(ValueError):
            ch.sdust_intervals(64, 20, piece=piece)
    ch.close()
    empty = chunkpass.ReadChunk([], lib=lib)
    empty.sdust(64, 20, split="pieces")
    assert empty.n_serial == 0 and empty.sdust_intervals()[1].shape == (0, 2)
    empty.close()


# ---- 4. the intervals -------------------------------------------------------------------------------------------------------
def check_intervals(lib):
    w, t = 20, 12
    rng = np.random.default_rng(9)
    seqs = edge_reads(w, 2 * w + 2) + [rand_seq(rng, 100) + "N" + "A" * 200, "CA" * 40 + rand_seq(rng, 900) + "T" * 33]
    ch = load(lib, seqs)
    lists = []
    for piece in (2 * w + 2, 1 << 30):                              # tiny pieces; pieces longer than any read
        ch.sdust(w, t, split="pieces", piece=piece)                 # (the split call before it, which flags short reads, leaves nothing behind)
        iv_off, iv, flagged = ch.sdust_intervals(w, t, piece)
        masked, _, _ = ch.sdust(w, t)
        per_read = []
        for i, s in enumerate(seqs):
            x = iv[int(iv_off[i]):int(iv_off[i + 1])]
            per_read.append(x.tolist())
            if flagged[i]:
                assert x.shape[0] == 0
                continue
            assert (x[:, 0] < x[:, 1]).all() and (x[:, 0] >= 0).all() and (x[:, 1] <= len(s)).all()
            assert (x[1:, 0] > x[:-1, 1]).all()                     # ascending, disjoint and not adjacent
            assert int((x[:, 1] - x[:, 0]).sum()) == int(masked[i])
        lists.append((per_read, flagged.tolist()))
    assert lists[0] == lists[1]
    assert lists[0][1] == [False] * (len(seqs) - 2) + [True, False]
    assert sum(len(x) for x in lists[0][0]) > 10
    ch.close()


# ---- 5. the launch cap ------------------------------------------------------------------------------------------------------
def check_pieces_past_cap(lib):
    masked_of = oracle_masked()
    cap, block = header_define("LQ_DUST_SPLIT_MAX_THREADS"), header_define("LQ_DUST_THREADS")
    w, t = 8, 5
    piece = 2 * w + 2
    rng = np.random.default_rng(51)
    lens, seqs = [], []
    n_items = 0
    while n_items < cap + 3000:
        n = int(rng.integers(split_min(piece), 900))
        k = rng.random()
        if k < 0.5:
            s = rand_seq(rng, n)
        elif k < 0.8:
            u = rand_seq(rng, int(rng.integers(1, 4)))
            s = rand_seq(rng, n // 3) + (u * n)[:n - n // 3]
        else:
            s = "".join("GT"[int(x)] for x in rng.integers(0, 2, n))
        if rng.random() < 0.02:
            s = s[:n // 2] + "N" + s[n // 2 + 1:]                    # (a flagged read between the others: no items)
        else:
            n_items += (n + piece - 1) // piece
        seqs.append(s)
    if n_items % block == 0:
        seqs.append("ACG" * 20); n_items += (60 + piece - 1) // piece
    assert_past_cap("k_sdust_pieces, (read, piece) items", n_items, cap, block)
    print("%d reads, %d bases, %d items of %d bases, %d reads with an N" % (len(seqs), sum(map(len, seqs)), n_items, piece, sum("N" in s for s in seqs)))
    ch = load(lib, seqs)
    got, _, _ = ch.sdust(w, t, split="pieces", piece=piece)
    assert ch.n_serial == sum(1 for s in seqs if "N" in s) > 10
    serial, _, _ = ch.sdust(w, t)
    ch.close()
    n = len(seqs)
    assert got[:n].tolist() == serial[:n].tolist()
    items = np.cumsum([0 if "N" in s else (len(s) + piece - 1) // piece for s in seqs])
    second = np.flatnonzero(items > cap)                            # reads with items of the second round
    sample = np.concatenate([second[:150], second[-150:], rng.choice(second[0], 300, replace=False)])
    assert [int(got[i]) for i in sample] == [masked_of(seqs[i], w, t) for i in sample]
    assert (got[second] > 0).sum() > 100 and got[:n].sum() > 0.2 * sum(len(s) for s in seqs)


# ---- 6. the halo matters ----------------------------------------------------------------------------------------------------
def test_a_halo_of_half_a_window_loses_the_straddling_interval(emu_lib, tmp_path):
    """the emulator library built again with LQ_DUST_SPLIT_HALO(W) = W / 2 (dust.cpp and chunk.cpp alone, the rest of the library comes
    from the session's build): the reads with a perfect interval over a piece border no longer give the oracle's counts"""
    so = str(tmp_path / "liblqcov_halo.so")
    emu = os.path.join(ROOT, "tests", "emu")
    r = subprocess.run(["g++", "-DLQ_EMU", "-DLQ_DUST_SPLIT_HALO(W)=((W)/2)", "-include", os.path.join(emu, "hipemu.hpp"), "-O1", "-std=c++17", "-fPIC",
                        "-Wno-unknown-pragmas", "dust.cpp", "chunk.cpp", "-shared", "-o", so, os.path.join(emu, "liblqcov_emu.so"),
                        "-Wl,-rpath," + emu, "-lz"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    lib = C.CDLL(so)
    chunkpass._lib(lib)
    masked_of = oracle_masked()
    w, t, piece = 64, 20, 130
    seqs = edge_reads(w, piece)
    want = [masked_of(s, w, t) for s in seqs]
    got = {}
    for tag, l in (("short halo", lib), ("halo of 2 W + 2", emu_lib)):
        ch = load(l, seqs)
        try:
            got[tag] = ch.sdust(w, t, split="pieces", piece=piece)[0][:len(seqs)].tolist()
            assert ch.n_serial == 0                                 # every read was cut, in both builds
        finally:
            ch.close()
    print("oracle", want, got)
    assert got["halo of 2 W + 2"] == want
    # the reads whose low-complexity stretch begins at a piece border, after a random piece: the intervals over that border are lost.
    # (Where the stretch goes on over many borders, as in read 3, the later pieces' intervals cover what one piece loses.)
    assert got["short halo"][5] < want[5] and got["short halo"][6] < want[6]


# ---- the emulator build -----------------------------------------------------------------------------------------------------
def test_emulated_split_golden_tables(emu_lib):
    check_golden(emu_lib)


@pytest.mark.parametrize("order", ORDERS)
def test_emulated_split_edge_reads(emu_lib, monkeypatch, order):
    set_order(monkeypatch, order)
    check_edges(emu_lib)


def test_emulated_split_serial_routing(emu_lib):
    check_serial_routing(emu_lib)


def test_emulated_split_errors_and_empty_chunk(emu_lib):
    check_errors(emu_lib)


@pytest.mark.parametrize("order", ORDERS)
def test_emulated_split_intervals(emu_lib, monkeypatch, order):
    set_order(monkeypatch, order)
    check_intervals(emu_lib)


def test_emulated_split_pieces_past_the_cap(emu_lib):
    check_pieces_past_cap(emu_lib)


def test_emulated_sdust_main_honours_the_switch(emu_lib, tmp_path, monkeypatch):
    from tests.test_sdust import check_main_equals_fixture
    monkeypatch.setenv("LQSDUST_SPLIT", "pieces")
    assert sdust.split_mode(None) == chunkpass.split_mode(None) == "pieces"
    for case in CASES[:2]:
        check_main_equals_fixture(emu_lib, case, tmp_path)
    monkeypatch.setenv("LQSDUST_SPLIT", "halves")
    with pytest.raises(ValueError):
        sdust.split_mode(None)
    from tests.test_sdust import run_sdust_main
    rc, _, err = run_sdust_main(emu_lib, CASES[0]["argv"], cwd=GOLDEN, tmp=tmp_path)
    assert rc != 0 and "LQSDUST_SPLIT" in err


# ---- the gfx950 build -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_split_golden_tables(gpu_lib):
    check_golden(gpu_lib)


@pytest.mark.gpu
def test_gpu_split_edge_reads(gpu_lib):
    check_edges(gpu_lib)


@pytest.mark.gpu
def test_gpu_split_serial_routing_and_errors(gpu_lib):
    check_serial_routing(gpu_lib)
    check_errors(gpu_lib)


@pytest.mark.gpu
def test_gpu_split_intervals(gpu_lib):
    check_intervals(gpu_lib)


@pytest.mark.gpu
def test_gpu_split_pieces_past_the_cap(gpu_lib):
    check_pieces_past_cap(gpu_lib)


def synthetic_reads(n=2000, seed=77):
    """n reads of 200..20 000 bases, a tenth of the bases in low-complexity inserts, one read in a hundred with an N"""
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(n):
        l = int(rng.integers(200, 20001))
        s = ACGT[rng.integers(0, 4, l)]
        at = 0
        while at < l:
            at += int(rng.integers(200, 1800))
            m = int(rng.integers(20, 200))
            if at + m >= l:
                break
            u = ACGT[rng.integers(0, 4, int(rng.integers(1, 5)))]
            s[at:at + m] = np.tile(u, m // len(u) + 1)[:m]
            at += m
        if rng.random() < 0.01:
            s[rng.integers(0, l)] = ord("N")
        seqs.append(s.tobytes().decode())
    return seqs


@pytest.mark.gpu
def test_gpu_split_equals_serial_on_a_synthetic_set_at_the_default_piece(gpu_lib):
    seqs = synthetic_reads()
    rng = np.random.default_rng(5)
    quals = ["".join(map(chr, 33 + rng.integers(2, 45, len(s)))) for s in seqs]
    ch = load(gpu_lib, seqs, quals)
    want = ch.sdust()
    got = ch.sdust(split="pieces")
    for g, x, what in zip(got, want, ("masked", "psum", "qv")):
        assert g.tobytes() == x.tobytes(), what
    flagged = sum(1 for s in seqs if "N" in s or len(s) < split_min(sdust.SPLIT_PIECE))
    assert ch.n_serial == flagged and 0 < flagged < len(seqs) // 2
    assert want[0].sum() > 0.05 * sum(len(s) for s in seqs)
    ch.close()


def check_run_file(lib, tmp_path):
    path = os.path.join(GOLDEN, "tiny_all.fq.gz")
    tables = []
    for tag, split in (("a", None), ("b", "pieces")):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "pb-sequel", nsample=40, inds=200000, gc_seed=3, suffix="x", lib=lib)
        np.random.seed(11)
        p.run_file(path, sdust_split=split)
        p.mask.close_pool()
        tables.append(open(p.mask.get_outfile_path(), "rb").read())
        assert p.mask.split == "serial"                             # sdust_split held for that file: the constructor's mode is back
        p.close()
    assert tables[0] == tables[1] == read_gz("tiny_all.sdust.gz").encode()


def test_emulated_run_file_table_with_pieces_equals_the_default_table(emu_lib, tmp_path):
    check_run_file(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_run_file_table_with_pieces_equals_the_default_table(gpu_lib, tmp_path):
    check_run_file(gpu_lib, tmp_path)

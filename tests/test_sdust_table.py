"""The low-complexity table formatted on the device (kernels_dust_table.hpp: k_sdust_rows, k_sdust_patch, k_sdust_text; lqsdust_format,
lqchunk_sdust_table; ReadChunk.sdust_table, LqMaskMI355X(table="device"), summary()) against the host path, sdust._rows, and the reference's
committed tables.
  1. lq_fmt3_round against Python's "%.3f" (the same correctly rounded conversion), on the host;
  2. lqsdust_format against _rows: seeded rows around every special case, crafted unvouched rows, the cap on random rows, window = 1;
  3. the exclusion lists just on either side of both thresholds, from lqsdust_format's stats and lqsdust_format_lists' indices; the host
     mode's sdust.exclusion_lists against the rule on the printed text;
  4. the golden tables through FileChunks / ReadChunk + sdust_table, both scan forms;
  5. device mode end to end: LqMaskMI355X (hand-made reads with both lists' neighbours, and tiny_all.fq.gz) and SampleQCPass.run_file, the
     file and summary() against host mode and a restatement;
  6. refusals;
  7. (GPU only) 200 000 random rows: the device's log10 against glibc's.
A FASTA file read by FileChunks carries '!' qualities (the reader's rule), so its meanQ column is not the reference's "-nan": the FASTA
cases go through ReadChunk from lists, which holds no quality buffer for them."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from longqc_amd import api, chunkpass, sampleqc, sdust
from tests import test_launch_caps as LC
from tests.conftest import GOLDEN, read_gz
from tests.helpers import read_fastx

CASES = json.load(open(os.path.join(GOLDEN, "sdust_cases.json")))
ADP5, ADP3 = sampleqc.PRESET_ADAPTERS["ont-ligation"]
I31 = 2 ** 31 - 1


class QFirst:
    """what _rows asks a quality buffer, for rows that have no reads behind them: the byte at a read's first base (reads with bases
    start at distinct offsets; _rows does not ask for the others)"""

    def __init__(self, off, lens, has_q):
        self.at = {int(o): int(h) for o, l, h in zip(off[:-1].tolist(), lens.tolist(), has_q.tolist()) if l}

    def __getitem__(self, k):
        return self.at[k]


def want_text(names, masked, lens, psum, has_q, qv):
    """the host path's text for arrays"""
    n = len(names)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens.astype(np.uint64), out=off[1:])
    rows = sdust._rows(names, n, off, QFirst(off, lens, has_q), masked, psum, qv)
    return ("\n".join(rows) + "\n").encode() if n else b""


def rand_names(rng, n):
    out = ["".join(chr(x) for x in rng.integers(48, 123, int(l))) for l in rng.integers(0, 41, n)]
    out[0], out[1] = "", "".join(chr(x) for x in rng.integers(48, 123, 40))
    return out


def seeded_rows(seed, n=4096):
    """-> names, masked, lens, psum, has_q, qv: random rows, and in turn rows whose fraction is an exact half of a thousandth in binary
    (1/16, 3/16), (2k + 1) / 2000 and its two neighbours, empty reads, reads without qualities, psum == len, psum / len down to 1e-12,
    ten-digit counts"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 60000, n).astype(np.int64)
    masked = (lens * rng.random(n)).astype(np.int64)
    psum = lens * 10.0 ** (-rng.random(n) * 4)
    has_q = np.ones(n, np.uint8)
    qv = (lens * rng.random(n)).astype(np.int64)
    for i in range(n):
        k = i % 16
        if k == 1:                                                  # 1/16 = 0.0625 -> 0.062, 3/16 = 0.1875 -> 0.188 (ties to even)
            j = int(rng.integers(1, 4000))
            lens[i], masked[i] = 16 * j, (1 if i % 32 == 1 else 3) * j
        elif k in (2, 3, 4):                                        # (2k + 1) / 2000: a half in decimal, a neighbour of one in binary
            j, h = int(rng.integers(1, 30)), int(rng.integers(0, 1000))
            lens[i], masked[i] = 2000 * j, (2 * h + 1) * j + (k - 3)
        elif k == 5:
            lens[i] = masked[i] = qv[i] = 0
            has_q[i] = i % 32 == 5                                  # (qualities claimed for a read without bases: none, _rows' rule)
        elif k == 6:
            has_q[i] = 0
        elif k == 7:
            psum[i] = float(lens[i])                                # -0.000
        elif k == 8:
            psum[i] = lens[i] * 10.0 ** (-rng.random() * 12)
        elif k == 9:
            lens[i] = int(rng.integers(10 ** 9, I31 + 1))
            masked[i] = int(rng.integers(10 ** 9, lens[i] + 1))
            qv[i] = int(rng.integers(10 ** 9, I31 + 1))
            psum[i] = lens[i] * 10.0 ** (-rng.random() * 12)
    masked = np.clip(masked, 0, None)
    return rand_names(rng, n), masked.astype(np.uint32), lens.astype(np.uint32), psum, has_q, qv.astype(np.uint32)


def assert_same_text(got, want):
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        raise AssertionError("%d rows differ (%d and %d rows), the first: %r != %r" % (
            len(bad) + abs(len(g) - len(w)), len(g), len(w), g[bad[0]] if bad else None, w[bad[0]] if bad else None))


# ---- 1. the rounding ----
def check_fmt3(lib):
    rng = np.random.default_rng(3)
    xs = [0.0, -0.0, 0.0625, 0.1875, 0.5, 1.0, 0.0005, 0.0015, 0.9995, 123.4565, 1e-12, 5e-324, 2.0 ** -11, 2.0 ** -64, 2.0 ** -70, 2.0 ** 50 - 0.125]
    for k in rng.integers(0, 200000, 3000).tolist():                # halves of a thousandth and their neighbours
        h = (2 * k + 1) / 2000
        xs += [h, math.nextafter(h, 0), math.nextafter(h, 1e9)]
    xs += (rng.random(20000) * 10.0 ** rng.integers(-6, 5, 20000)).tolist()
    xs += [v for v in np.frombuffer(rng.integers(0, 2 ** 63, 20000).astype(np.uint64).tobytes(), np.float64).tolist() if math.isfinite(v)]      # any exponent
    xs += (2.0 ** 50 * (1 + rng.random(200))).tolist() + [2.0 ** 50, 1e300]
    n_big = 0
    for x in xs:
        for v in (x, -x):
            cls, thou = sdust.fmt3(v, lib=lib)
            if abs(v) >= 2.0 ** 50:
                assert cls == 3 + (4 if math.copysign(1, v) < 0 else 0)
                n_big += 1
                continue
            assert cls & 3 == 0
            text = ("-" if cls & 4 else "") + "%d.%03d" % (thou // 1000, thou % 1000)
            assert text == "%.3f" % v, (v, text)
    assert n_big > 100
    assert sdust.fmt3(math.nan, lib=lib)[0] & 3 == 1 and sdust.fmt3(math.inf, lib=lib) == (2, 0) and sdust.fmt3(-math.inf, lib=lib) == (6, 0)


def test_emulated_rounding_equals_printf(emu_lib):
    check_fmt3(emu_lib)


# ---- 2. lqsdust_format ----
def check_format(lib):
    names, masked, lens, psum, has_q, qv = seeded_rows(17)
    want = want_text(names, masked, lens, psum, has_q, qv)
    for col, pat in ((3, b"-nan"), (4, b"-nan"), (4, b"-0.000"), (3, b"0.062"), (3, b"0.188")):
        assert sum(r.split(b"\t")[col] == pat for r in want.split(b"\n")[:-1]) >= 50, pat
    assert max(float(r.split(b"\t")[4]) for r in want.split(b"\n")[:-1] if b"nan" not in r.split(b"\t")[4]) > 100
    got, st = sdust.format_rows(names, masked, lens, psum, has_q, qv, lib=lib)
    assert_same_text(got, want)
    n = len(names)
    assert st["rows"] == n and st["bytes"] == len(want) and st["masked"] == int(masked.sum(dtype=np.uint64)) and st["q7"] == int(qv.sum(dtype=np.uint64))
    print("unvouched among %d seeded rows: %d" % (n, st["unvouched"]))
    assert st["unvouched"] <= n // 100
    assert len(want) <= sum(len(x) for x in names) + sdust.ROW_FIELDS_MAX * n
    # window = 1: every row with qualities takes the host's meanQ, and the text is the same
    got1, st1 = sdust.format_rows(names, masked, lens, psum, has_q, qv, window=1.0, lib=lib)
    assert st1["unvouched"] == int(((has_q != 0) & (lens > 0)).sum()) and st1["unvouched"] > n // 2
    assert_same_text(got1, want)
    assert {k: v for k, v in st1.items() if k != "unvouched"} == {k: v for k, v in st.items() if k != "unvouched"}
    # has_q NULL: no row has qualities
    got0, st0 = sdust.format_rows(names, masked, lens, psum, None, qv, lib=lib)
    assert_same_text(got0, want_text(names, masked, lens, psum, np.zeros(n, np.uint8), qv))
    assert st0["unvouched"] == 0
    # no rows
    assert sdust.format_rows([], [], [], [], [], [], lib=lib) == (b"", dict(dict.fromkeys(st, 0), exclude_first=[], exclude_second=[]))


def check_crafted_unvouched(lib):
    """psum = len * 10^(-(k + 0.5) / 10000): meanQ * 1000 = k + 0.5 up to the libraries' error -- all reported, and printed as _rows does"""
    rng = np.random.default_rng(23)
    n = 200
    ks = rng.integers(0, 60000, n)
    lens = rng.integers(1, 60000, n).astype(np.uint32)
    psum = lens * 10.0 ** (-(ks + 0.5) / 10000)
    names = ["k%d" % k for k in ks.tolist()]
    masked, qv, has_q = (lens // 3).astype(np.uint32), (lens // 2).astype(np.uint32), np.ones(n, np.uint8)
    got, st = sdust.format_rows(names, masked, lens, psum, has_q, qv, lib=lib)
    assert st["unvouched"] == n
    assert_same_text(got, want_text(names, masked, lens, psum, has_q, qv))


def check_random_cap(lib, n):
    """random (psum, len): at most 1 % may be unvouched (the numpy restatement of the window marks about 2 in 100 000) -- and zero
    rows differ from _rows"""
    rng = np.random.default_rng(29)
    lens = rng.integers(1, 100000, n).astype(np.uint32)
    psum = lens * 10.0 ** (-rng.random(n) * 5)
    masked, qv, has_q = (lens * rng.random(n)).astype(np.uint32), (lens * rng.random(n)).astype(np.uint32), np.ones(n, np.uint8)
    names = ["r%d" % i for i in range(n)]
    got, st = sdust.format_rows(names, masked, lens, psum, has_q, qv, lib=lib)
    print("unvouched among %d random rows: %d" % (n, st["unvouched"]))
    assert st["unvouched"] <= n // 100
    assert_same_text(got, want_text(names, masked, lens, psum, has_q, qv))


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_format_equals_rows(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_format(emu_lib)
    check_crafted_unvouched(emu_lib)
    check_random_cap(emu_lib, 3000)


@pytest.mark.gpu
def test_gpu_format_equals_rows(gpu_lib):
    check_format(gpu_lib)
    check_crafted_unvouched(gpu_lib)
    check_random_cap(gpu_lib, 3000)


@pytest.mark.gpu
def test_gpu_log10_against_glibc_on_200000_rows(gpu_lib):
    check_random_cap(gpu_lib, 200000)


# ---- 3. the exclusion lists ----
def check_exclusion(lib):
    rng = np.random.default_rng(31)
    lens, masked = [], []
    for ln in (10000, 10001, 500000, 500001):
        for thou in (200, 201, 400, 401):                           # every masked count that prints as 0.200 .. 0.401
            lo, hi = math.ceil((thou - 0.5) * ln / 1000), math.floor((thou + 0.5) * ln / 1000)
            for m in (lo, (lo + hi) // 2, hi):
                lens.append(ln); masked.append(m)
    lens += [0, 0, 9999, 20000, 600000, 600000, 20000]              # "-nan" rows, a short read, reads far inside and far outside
    masked += [0, 0, 9999, 20000, 600000, 1000, 100]
    n = len(lens)
    perm = rng.permutation(n)
    lens, masked = np.array(lens, np.uint32)[perm], np.array(masked, np.uint32)[perm]
    psum, has_q, qv = lens * 0.01, np.ones(n, np.uint8), (lens // 2).astype(np.uint32)
    names = ["e%d" % i for i in range(n)]
    got, st = sdust.format_rows(names, masked, lens, psum, has_q, qv, lib=lib)
    assert_same_text(got, want_text(names, masked, lens, psum, has_q, qv))
    rows = [r.split("\t") for r in got.decode().splitlines()]
    printed = {r[3] for r in rows}
    assert {"0.200", "0.201", "0.400", "0.401", "-nan"} <= printed
    first = [r[0] for r in rows if int(r[2]) > 500000 and float(r[3]) > 0.2]      # longQC.py:370-371 on what pandas would parse
    second = [r[0] for r in rows if int(r[2]) > 10000 and float(r[3]) > 0.4]
    assert len(first) >= 10 and len(second) >= 10 and set(first) & set(second) and set(first) - set(second) and set(second) - set(first)
    assert any(r[3] == "0.200" and int(r[2]) == 500001 for r in rows) and any(r[3] == "0.201" and int(r[2]) == 500000 for r in rows)
    assert st["excluded_first"] == len(first) and st["excluded"] == len(first) + len(second)
    # the device's lists (lqsdust_format_lists): the first, then the second behind it, each in file order whatever order the atomics took
    assert [names[i] for i in st["exclude_first"]] == first and [names[i] for i in st["exclude_second"]] == second
    f2, s2 = sdust.exclusion_lists(masked, lens)                    # the host mode's lists: the same reads
    assert [names[i] for i in f2] == first and [names[i] for i in s2] == second
    # excl_cap one short of the lists: refused, nothing written
    nb, noff = api.encode_names(names)
    out, n_out, excl, err = np.full(len(got), 0xEE, np.uint8), C.c_uint64(), np.full(len(first) + len(second), 0xEEEEEEEE, np.uint32), C.create_string_buffer(512)
    rc = sdust._lib(lib).lqsdust_format_lists(0, n, nb, noff.ctypes.data, masked.ctypes.data, lens.ctypes.data, psum.ctypes.data, has_q.ctypes.data,
                                              qv.ctypes.data, 0.0, out.ctypes.data, len(got), C.byref(n_out), None, excl.ctypes.data, excl.size - 1, err, 512)
    assert rc == -1 and b"excl_cap" in err.value and (out == 0xEE).all() and (excl == 0xEEEEEEEE).all()
    rc = sdust._lib(lib).lqsdust_format_lists(0, n, nb, noff.ctypes.data, masked.ctypes.data, lens.ctypes.data, psum.ctypes.data, has_q.ctypes.data,
                                              qv.ctypes.data, 0.0, out.ctypes.data, len(got), C.byref(n_out), None, excl.ctypes.data, excl.size, err, 512)
    assert rc == 0 and out.tobytes() == got and excl.tolist() == st["exclude_first"] + st["exclude_second"]


def test_host_exclusion_lists_follow_the_printed_fraction():
    """sdust.exclusion_lists (host mode's, array work alone) against the rule on the text: every masked count around both borders at many
    lengths, where masked / len is within a few thousandths of 0.2005 and 0.4005"""
    rng = np.random.default_rng(43)
    lens, masked = [], []
    for ln in [10000, 10001, 500000, 500001, 2000000, 4000000, I31] + rng.integers(10001, 3000000, 3000).tolist():
        for border in (0.2005, 0.4005):
            m = int(border * ln)
            for d in range(-2, 4):
                lens.append(ln); masked.append(m + d)
    for j in rng.integers(6, 1000, 500).tolist():                   # masked / len == 0.2005 and 0.4005 in decimal: the nearest double decides
        lens += [2000 * j, 2000 * j]; masked += [401 * j, 801 * j]
    lens, masked = np.array(lens, np.uint32), np.array(masked, np.uint32)
    thou = [round(float("%.3f" % (int(m) / int(l))) * 1000) for m, l in zip(masked.tolist(), lens.tolist())]
    first = [i for i, (t, l) in enumerate(zip(thou, lens.tolist())) if l > 500000 and t > 200]
    second = [i for i, (t, l) in enumerate(zip(thou, lens.tolist())) if l > 10000 and t > 400]
    assert {200, 201, 400, 401} <= set(thou) and len(first) > 1000 and len(second) > 1000
    assert sdust.exclusion_lists(masked, lens) == (first, second)
    assert sdust.exclusion_lists(np.zeros(0, np.uint32), np.zeros(0, np.int64)) == ([], [])


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_exclusion_lists(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_exclusion(emu_lib)


@pytest.mark.gpu
def test_gpu_exclusion_lists(gpu_lib):
    check_exclusion(gpu_lib)


# ---- 4. the golden tables ----
def case_args(case):
    """-> (file, w, t) of a case's argv (-w 32, -w32)"""
    w, t, fn, a = 64, 20, None, list(case["argv"])
    while a:
        x = a.pop(0)
        if x[:2] in ("-w", "-t"):
            v = int(x[2:] or a.pop(0))
            w, t = (v, t) if x[1] == "w" else (w, v)
        else:
            fn = x
    return fn, w, t


def check_golden(lib, case):
    fn, w, t = case_args(case)
    want = read_gz(case["expect"]).encode()
    path = os.path.join(GOLDEN, fn)
    names, seqs, quals = read_fastx(path)
    reads = [[nm, bytes(s), bytes(q) if q is not None and len(q) else None] for nm, s, q in zip(names, seqs, quals if quals is not None else [None] * len(seqs))]
    for split in (None, "pieces"):
        ch = chunkpass.ReadChunk(reads, lib=lib)
        got, st = ch.sdust_table(w, t, split=split)
        ch.close()
        assert_same_text(got, want)
        assert st["rows"] == len(reads) and st["bytes"] == len(want) and st["masked"] == case["masked_total"]
        if ".fq" in fn:                                             # through the reader, in several chunks
            parts, n_chunks = [], 0
            for ch, _, _ in chunkpass.FileChunks(path, chunk_size=5000, is_upper=False, lib=lib):
                parts.append(ch.sdust_table(w, t, split=split)[0])
                n_chunks += 1
            assert n_chunks >= 2
            assert_same_text(b"".join(parts), want)
    if fn == "adv_all.fa.gz":
        assert b"\t-nan\t" in want


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_emulated_golden_tables(emu_lib, case):
    check_golden(emu_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_gpu_golden_tables(gpu_lib, case):
    check_golden(gpu_lib, case)


# ---- 5. device mode end to end ----
def restated_summary(path):
    """longQC.py:369-371, 452-471 on the written file, without pandas"""
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    lens = [int(r[2]) for r in rows]
    excl = [r[0] for r in rows if int(r[2]) > 500000 and float(r[3]) > 0.2] + [r[0] for r in rows if int(r[2]) > 10000 and float(r[3]) > 0.4]
    n50, cnt = None, 0
    for x in sorted(lens, reverse=True):                            # lq_utils.get_N50
        cnt += x
        if cnt >= sum(lens) / 2:
            n50 = x
            break
    return {"n_reads": len(lens), "yield": sum(lens), "longest": max(lens), "mean_length": float(np.array(lens).mean()), "n50": n50,
            "q7_bases": sum(int(r[5]) for r in rows), "masked_bases": sum(int(r[1]) for r in rows), "exclude_seqs": excl}


def check_mask_modes(lib, tmp_path):
    rng = np.random.default_rng(37)

    def read(name, seq):
        return [name, seq, "".join(chr(x) for x in rng.integers(34, 80, len(seq)))]
    rnd = lambda l: "".join("ACGT"[x] for x in rng.integers(0, 4, l))
    chunks = [[read("a", rnd(700)), read("polyA", "A" * 10001), read("", rnd(30)), read("at10000", "AT" * 5000), read("empty", "")],
              [read("half", "AC" * 3000 + rnd(6001)), read("polyA", "A" * 10500), ["bare", rnd(900)], read("rnd", rnd(12000))]]
    out = {}
    for mode in ("host", "device"):
        for resident in (False, True):
            m = sdust.LqMaskMI355X(str(tmp_path / ("%s%d" % (mode, resident))), suffix="x", lib=lib, table=mode)
            for k, reads in enumerate(chunks):
                if resident:
                    ch = chunkpass.ReadChunk(reads, lib=lib)
                    m.submit_sdust(None, k, chunk=ch)
                    ch.close()
                else:
                    m.submit_sdust(reads, k)
            s = m.summary()
            m.close_pool()
            assert m.summary() == s                                 # (kept beyond close_pool)
            out[mode, resident] = (open(m.get_outfile_path(), "rb").read(), s, m.json_block())
    ref = out["host", False]
    assert all(v == ref for v in out.values())
    path = str(tmp_path / "host0" / "longqc_sdust_x.txt")
    want = restated_summary(path)
    assert ref[1] == want
    # no read is over 500 000; "half" is 12 001 bases whose first 6 000 are a masked AC repeat (6028 masked, 0.502), in file order between the two
    assert want["exclude_seqs"] == ["polyA", "half", "polyA"], want["exclude_seqs"]
    assert "polyA" in want["exclude_seqs"] and "at10000" not in want["exclude_seqs"] and "rnd" not in want["exclude_seqs"]
    assert ref[2] == {"Yield": want["yield"], "Q7 bases": "%.2f%%" % float(100 * want["q7_bases"] / want["yield"]), "Longest_read": want["longest"],
                      "Num_of_reads": want["n_reads"], "Length_stats": {"Mean_read_length": want["mean_length"], "N50_read_length": float(want["n50"])}}
    with pytest.raises(ValueError):
        sdust.LqMaskMI355X(str(tmp_path / "bad"), lib=lib, table="gpu")


def check_mask_tiny_all(lib, tmp_path):
    """LqMaskMI355X(table="device") on tiny_all.fq.gz, in chunks of 7 reads, from records and from resident chunks: the reference's table,
    host mode's summary, and the restatement on the written file"""
    names, seqs, quals = read_fastx(os.path.join(GOLDEN, "tiny_all.fq.gz"))
    reads = [[nm, bytes(s), bytes(q)] for nm, s, q in zip(names, seqs, quals)]
    chunks = [reads[i:i + 7] for i in range(0, len(reads), 7)]
    assert len(chunks) >= 3
    out = {}
    for mode in ("host", "device"):
        for resident in (False, True):
            m = sdust.LqMaskMI355X(str(tmp_path / ("tiny_%s%d" % (mode, resident))), lib=lib, table=mode)
            for k, part in enumerate(chunks):
                if resident:
                    ch = chunkpass.ReadChunk(part, lib=lib)
                    m.submit_sdust(None, k, chunk=ch)
                    ch.close()
                else:
                    m.submit_sdust(part, k)
            m.close_pool()
            out[mode, resident] = (open(m.get_outfile_path(), "rb").read(), m.summary(), m.json_block())
    assert out["device", True][0] == read_gz("tiny_all.sdust.gz").encode()
    assert all(v == out["device", True] for v in out.values())
    assert out["device", True][1] == restated_summary(str(tmp_path / "tiny_device1" / "longqc_sdust.txt"))


def check_run_file_modes(lib, tmp_path, monkeypatch):
    path = os.path.join(GOLDEN, "tiny_all.fq.gz")
    kw = dict(adp5=ADP5, adp3=ADP3, nsample=15, gc_draw="device", gc_seed=3, suffix="x", lib=lib)
    res = {}
    for tag, ctor, call in (("host", {}, {}), ("device", {}, {"sdust_table": "device"}), ("ctor", {"sdust_table": "device"}, {}),
                            ("pieces", {"sdust_split": "pieces"}, {"sdust_table": "device"})):
        p = chunkpass.SampleQCPass(str(tmp_path / tag), "ont-ligation", **kw, **ctor)
        if tag == "device":                                         # no row becomes a Python string on the way
            monkeypatch.setattr(sdust, "_rows", lambda *a, **k: 1 / 0)
        np.random.seed(11)
        r = p.run_file(path, chunk_size=100000, str_overhead=49, **call)
        monkeypatch.undo()
        assert p.mask.table == ("device" if tag == "ctor" else "host")         # (run_file's mode held for the file)
        assert len(r) >= 3
        p.mask.close_pool()
        res[tag] = (open(p.mask.get_outfile_path(), "rb").read(), p.summary(), p.mask.json_block(), p.s_reads, p.gc.json_block())
        p.close()
    assert all(v == res["host"] for v in res.values())
    assert res["host"][0] == read_gz("tiny_all.sdust.gz").encode()
    assert res["host"][1] == restated_summary(str(tmp_path / "host" / "longqc_sdust_x.txt"))
    monkeypatch.setenv("LQSDUST_TABLE", "device")
    assert sdust.table_mode(None) == "device" and sdust.LqMaskMI355X(str(tmp_path / "env"), lib=lib).table == "device"
    monkeypatch.setenv("LQSDUST_TABLE", "nowhere")
    with pytest.raises(ValueError):
        sdust.table_mode(None)


@pytest.mark.parametrize("order", LC.ORDERS)
def test_emulated_mask_modes_agree(emu_lib, tmp_path, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_mask_modes(emu_lib, tmp_path)
    check_mask_tiny_all(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_mask_modes_agree(gpu_lib, tmp_path):
    check_mask_modes(gpu_lib, tmp_path)
    check_mask_tiny_all(gpu_lib, tmp_path)


def test_emulated_run_file_modes_agree(emu_lib, tmp_path, monkeypatch):
    check_run_file_modes(emu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_run_file_modes_agree(gpu_lib, tmp_path, monkeypatch):
    check_run_file_modes(gpu_lib, tmp_path, monkeypatch)


# ---- 6. refusals ----
def check_refusals(lib):
    rng = np.random.default_rng(41)
    recs = [["n%d" % i, "".join("ACGT"[x] for x in rng.integers(0, 4, l)), "5" * l] for i, l in enumerate((300, 0, 5000, 77))]
    ch = chunkpass.ReadChunk(recs, lib=lib)
    with pytest.raises(api.LqcovError) as e:                        # no scan yet
        ch.sdust_table_bytes()
    assert e.value.code == -4 and "scan" in str(e.value)
    want = ("\n".join(sdust.sdust_rows(ch.names, None, None, chunk=ch)) + "\n").encode()
    assert ch.sdust_table_bytes()[0] == want                        # (a scan that copied its arrays back serves as well)
    ch.load(recs[:3])                                               # a new load: the arrays on the device are the old chunk's
    with pytest.raises(api.LqcovError) as e:
        ch.sdust_table_bytes()
    assert e.value.code == -4
    ch.load(recs)
    for split in (None, "pieces"):                                  # NULL host arrays to both scan calls, then the table
        assert ch.sdust_table(split=split)[0] == want
    # a short out_cap: refused, nothing written, and the next call works
    lib_, (nb, noff) = ch.lib, ch.names_c()
    out, n_out, st = np.full(len(want) + 8, 0xEE, np.uint8), C.c_uint64(), (C.c_uint64 * 8)()
    excl = np.full(8, 0xEEEEEEEE, np.uint32)
    rc = lib_.lqchunk_sdust_table(ch.h, nb, noff.ctypes.data, out.ctypes.data, len(want) - 1, C.byref(n_out), st, excl.ctypes.data, 8)
    assert rc == -1 and "out_cap" in lib_.lqchunk_last_error(ch.h).decode()
    assert (out == 0xEE).all() and (excl == 0xEEEEEEEE).all() and n_out.value == len(want) and st[0] == len(recs)
    rc = lib_.lqchunk_sdust_table(ch.h, nb, noff.ctypes.data, out.ctypes.data, len(want), C.byref(n_out), st, excl.ctypes.data, 8)
    assert rc == 0 and out[:len(want)].tobytes() == want and (out[len(want):] == 0xEE).all()
    with pytest.raises(api.LqcovError) as e:
        ch.sdust_table_bytes(out_cap=10)
    assert e.value.code == -1
    # the three host arrays come together
    m = np.zeros(8, np.uint32)
    assert lib_.lqchunk_sdust(ch.h, 64, 20, m.ctypes.data, None, None) == -1
    assert lib_.lqchunk_sdust_split(ch.h, 64, 20, 0, None, None, m.ctypes.data, None) == -1
    # lqsdust_format: a short out_cap, a negative window
    with pytest.raises(api.LqcovError) as e:
        sdust.format_rows(["a", "b"], [1, 2], [10, 20], [1.0, 2.0], [1, 1], [3, 4], lib=lib, out_cap=20)
    assert e.value.code == -1
    with pytest.raises(api.LqcovError) as e:
        sdust.format_rows(["a"], [1], [10], [1.0], [1], [3], window=-1.0, lib=lib)
    assert e.value.code == -1
    assert sdust.format_rows(["a"], [1], [10], [10.0], [1], [3], lib=lib)[0] == b"a\t1\t10\t0.100\t-0.000\t3\n"
    # the same reads as arrays (load_arrays): the same table; offsets that do not fit the bases are refused
    seq = np.frombuffer("".join(r[1] for r in recs).encode(), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r[1]) for r in recs])]).astype(np.uint64)
    ch.load_arrays([r[0] for r in recs], seq, off, np.full(seq.shape[0], ord("5"), np.uint8))
    assert ch.sdust_table()[0] == want and ch.sdust_table(split="pieces")[0] == want
    assert ("\n".join(sdust.sdust_rows(ch.names, None, None, chunk=ch)) + "\n").encode() == want
    with pytest.raises(ValueError):
        ch.load_arrays([r[0] for r in recs], seq[:-1], off)
    # an empty chunk
    ch.load([])
    assert ch.sdust_table()[0] == b""
    ch.close()


def test_emulated_table_refusals(emu_lib):
    check_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_table_refusals(gpu_lib):
    check_refusals(gpu_lib)

"""The delimited-table reader (kernels_csv.hpp behind lqcsv_*, longqc_amd.rs.StsTable) field by field, under the wave emulator and on the GPU:

  * the four columns of every golden run directory (tests/golden/rs/, written and read with pd.read_table by make_rs_golden.py) equal
    pandas' recorded arrays bit for bit -- LF and CRLF, a last row without line break, blank lines, wanted columns in different
    places, a repeated column name, an all-integer ReadScore column read as int64 and as double;
  * the 20 020 recorded decimals inside the device's syntax (tests/golden/rs_decimals.txt.gz) all come from the device and equal
    float(text), which is correctly rounded;
  * numbers outside that syntax (an exponent, 16 and more digits, 23 decimals) go to the host twin -- the stats say so -- and equal
    float(text) as well;
  * everything outside the domain is refused with LQCOV_E_DOMAIN and the line number;
  * pieces of 64 bytes and smaller, where rows, fields and the "\\r\\n" pair straddle piece boundaries, and bytes that arrive in parts,
    give the same columns as one piece."""
import gzip
import json
import os

import numpy as np
import pytest

from longqc_amd import api, rs
from tests.conftest import GOLDEN

GOLD = json.load(open(os.path.join(GOLDEN, "rs.json")))
RUN_DIR = os.path.join(GOLDEN, "rs")
KIND = {"int64": rs.INT64, "float64": rs.DOUBLE}
OUTSIDE = ("1e-3", "1.5E2", "12345678901234567", "0.12345678901234567", "1E+22", "-2.5e-7", "1234567890123456", "0.00000000000000000000001",
           "9007199254740993", "4.35e+2", "1.e3", ".5e1", "-1234567890.1234567")
INSIDE = ("0.1", "-7", "123456789012345", ".25")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def want_columns(run):
    return {c: np.array(v["values"], dtype=v["dtype"]) for c, v in GOLD["runs"][run]["columns"].items()}


def read(lib, source, columns, **kw):
    with rs.StsTable(source, columns=columns, lib=lib, **kw) as t:
        return {n: t.column(n) for n, _ in columns}, dict(t.stats)


def check_golden_columns(lib):
    for run in GOLD["runs"]:
        want = want_columns(run)
        columns = [(c, KIND[str(a.dtype)]) for c, a in want.items()]
        got, st = read(lib, os.path.join(RUN_DIR, run, "m.sts.csv"), columns)
        for c, a in want.items():
            assert got[c].dtype == a.dtype and np.array_equal(bits(got[c]), bits(a)), (run, c)
        assert st["rows"] == len(want["NumBases"]) and st["fields_device"] == 4 * st["rows"] and st["fields_host"] == 0, (run, st)
    want = want_columns("intscore")                                   # the integer ReadScore column, converted: what rs.run_platformqc reads
    assert want["ReadScore"].dtype == np.int64
    got, _ = read(lib, os.path.join(RUN_DIR, "intscore", "m.sts.csv"), [("ReadScore", rs.DOUBLE)])
    assert np.array_equal(bits(got["ReadScore"]), bits(want["ReadScore"].astype(np.float64)))


def decimals():
    with gzip.open(os.path.join(GOLDEN, "rs_decimals.txt.gz"), "rb") as f:
        return f.read().decode().split()


def check_decimals(lib):
    texts = decimals()
    assert len(texts) >= 20000
    got, st = read(lib, ("x\n" + "\n".join(texts) + "\n").encode(), [("x", rs.DOUBLE)])
    want = np.array([float(t) for t in texts])
    bad = np.flatnonzero(bits(got["x"]) != bits(want))
    assert bad.size == 0, (bad.size, texts[bad[0]], got["x"][bad[0]].hex(), want[bad[0]].hex())
    assert st["fields_device"] == len(texts) and st["fields_host"] == 0, st


def check_twin(lib):
    texts = [t for pair in zip(OUTSIDE, INSIDE * 4) for t in pair]      # alternating: the twin's values land in their rows
    data = "k,x\n" + "".join("%d,%s\r\n" % (i, t) for i, t in enumerate(texts))
    got, st = read(lib, data.encode(), [("x", rs.DOUBLE), ("k", rs.INT64)])
    assert np.array_equal(bits(got["x"]), bits(np.array([float(t) for t in texts]))), [(t, g) for t, g in zip(texts, got["x"]) if float(t) != g]
    assert got["k"].tolist() == list(range(len(texts)))
    assert st["fields_host"] == len(OUTSIDE) and st["fields_device"] == 2 * len(texts) - len(OUTSIDE), st


ERRORS = (
    # the table, the wanted columns, the line, a piece of the reason
    ("a,b\n1,2\n3,\"4\"\n", [("a", rs.INT64)], 3, "quoted"),
    ("a,\"b\"\n1,2\n", [("a", rs.INT64)], 1, "quoted"),
    ("a,b\n1,2\n3\n", [("a", rs.INT64)], 3, "1 fields, the header has 2"),
    ("a,b\r\n1,2\r\n\r\n3,4,5\r\n", [("a", rs.INT64)], 4, "3 fields, the header has 2"),
    ("a,b\n1,\n", [("b", rs.INT64)], 2, "empty"),
    ("a,b\n1,2\n,2\n", [("a", rs.DOUBLE)], 3, "empty"),
    ("a,b\n1,2\nx,3\n", [("a", rs.INT64)], 3, "'x' is not a whole number"),
    ("a,b\n1,2\n1.5,3\n", [("a", rs.INT64)], 3, "not a whole number"),
    ("a,b\n1,2\n\n\n7,abc\n", [("b", rs.DOUBLE)], 5, "'abc' is not a plain number"),
    ("a,b\n1,nan\n", [("b", rs.DOUBLE)], 2, "'nan' is not a plain number"),
    ("a,b\n1,2\n1,-inf\n", [("b", rs.DOUBLE)], 3, "not a plain number"),
    ("a,b\n1, 2\n", [("b", rs.DOUBLE)], 2, "not a plain number"),
    ("a,b\n1,1e999\n", [("b", rs.DOUBLE)], 2, "not a finite double"),
    ("a,b\n1,2\n", [("c", rs.INT64)], 1, "no column 'c'"),
    ("a\n123456789012345678\n1234567890123456789\n", [("a", rs.INT64)], 3, "more than 18 digits"),
    ("a,b\n1\r2,3\n", [("a", rs.INT64)], 2, "'\\r'"),
    ("a,b\n1,2\n3,\x004\n", [("a", rs.INT64)], 3, "NUL"),
)


def check_errors(lib, tmp_path):
    for data, columns, line, why in ERRORS:
        for piece in (None, 5):
            with pytest.raises(api.LqcovError) as e:
                read(lib, data.encode(), columns, piece_bytes=piece)
            assert e.value.code == -5 and "line %d: " % line in str(e.value) and why in str(e.value), (data, str(e.value))
    # an unwanted column may hold any text without a quote; of a repeated name the first column counts
    got, _ = read(lib, b"a,t,a\n1,x y;z,5\n2,,6\n+3,-,7", [("a", rs.INT64)])
    assert got["a"].tolist() == [1, 2, 3]
    # from a file, the message names it; a file that is not there is an I/O error
    p = tmp_path / "bad.csv"
    p.write_bytes(b"a,b\n1,2\n3\n")
    with pytest.raises(api.LqcovError) as e:
        read(lib, str(p), [("a", rs.INT64)])
    assert e.value.code == -5 and "bad.csv" in str(e.value) and "line 3: " in str(e.value)
    with pytest.raises(api.LqcovError) as e:
        read(lib, str(tmp_path / "none.csv"), [("a", rs.INT64)])
    assert e.value.code == -2
    with pytest.raises(api.LqcovError) as e:                             # no header line at all
        read(lib, b"\n\r\n", [])
    assert e.value.code == -5
    got, st = read(lib, b"a,b\n", [("a", rs.INT64)])                     # a header and no rows
    assert got["a"].size == 0 and st["rows"] == 0


def check_pieces(lib):
    for run, pieces, steps in (("crlf", (64, 7), (13,)), ("intscore", (33,), (50,))):
        data = open(os.path.join(RUN_DIR, run, "m.sts.csv"), "rb").read()
        want = want_columns(run)
        columns = [(c, KIND[str(a.dtype)]) for c, a in want.items()]
        for piece in pieces:
            got, st = read(lib, data, columns, piece_bytes=piece)
            assert all(np.array_equal(bits(got[c]), bits(a)) for c, a in want.items()), (run, piece)
            assert st["pieces"] > 100 and st["bytes"] == len(data), (run, piece, st)
        for step in steps:                                           # the caller's own parts, cut anywhere: inside "\r\n" too
            parts = [data[i:i + step] for i in range(0, len(data), step)]
            assert run != "crlf" or any(p.endswith(b"\r") for p in parts)
            got, st = read(lib, parts, columns, piece_bytes=64)
            assert all(np.array_equal(bits(got[c]), bits(a)) for c, a in want.items()), (run, step)


def test_the_golden_file_holds_what_the_issue_names():
    pf = GOLD["pandas_float"]
    assert pf["n"] == 200000 and pf["differences"] == 0 and pf["naive_differences"] > 10000
    crlf = open(os.path.join(RUN_DIR, "crlf", "m.sts.csv"), "rb").read()
    assert crlf.count(b"\r\n") == crlf.count(b"\n") and b"\r\n\r\n" in crlf and not crlf.endswith(b"\n")
    assert crlf.split(b"\r\n")[0].split(b",").count(b"ReadScore") == 2
    lf = open(os.path.join(RUN_DIR, "lf", "m.sts.csv"), "rb").read()
    assert b"\r" not in lf and all(b"," + s + b"," in lf for s in (b"0.1", b"0.10", b"0.1000001"))
    assert GOLD["runs"]["intscore"]["columns"]["ReadScore"]["dtype"] == "int64"
    assert {len(t.partition(".")[2]) for t in decimals()} >= set(range(0, 23))


def test_emulated_columns_are_pandas(emu_lib):
    check_golden_columns(emu_lib)


def test_emulated_decimals_are_correctly_rounded(emu_lib):
    check_decimals(emu_lib)
    check_twin(emu_lib)


def test_emulated_domain_errors(emu_lib, tmp_path):
    check_errors(emu_lib, tmp_path)


def test_emulated_pieces(emu_lib):
    check_pieces(emu_lib)


def test_emulated_columns_do_not_depend_on_the_grid(emu_lib, monkeypatch):
    for blocks in ("1", "3"):                                           # every kernel strides: one block does what 256 do
        monkeypatch.setenv("LQCSV_TEST_MAX_BLOCKS", blocks)
        check_golden_columns(emu_lib)
        check_twin(emu_lib)


@pytest.mark.gpu
def test_gpu_columns_are_pandas(gpu_lib):
    check_golden_columns(gpu_lib)


@pytest.mark.gpu
def test_gpu_decimals_are_correctly_rounded(gpu_lib):
    check_decimals(gpu_lib)
    check_twin(gpu_lib)


@pytest.mark.gpu
def test_gpu_domain_errors(gpu_lib, tmp_path):
    check_errors(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_pieces(gpu_lib):
    check_pieces(gpu_lib)

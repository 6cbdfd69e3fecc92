"""The per-read figure data end to end, under the wave emulator and on the GPU: LqMaskMI355X keeps the two "%.3f" columns of its table as
thousandths (lqchunk_sdust_columns with table="device", the formatted rows otherwise) and gives the QV box plot by length bin and the
masked-fraction histogram of lq_mask.py:43-79 from them; CoverageTable gives the two grouped box plots of lq_coverage.py:438-529.

  * both table modes keep the same columns, and they are the file's: every field of longqc_sdust.txt parsed again with Decimal;
  * qscore_figure_data() equals test_boxstats.oracle (matplotlib's box, checked there) on the parsed file, by the interval rule of
    longQC.py:478-481 and by a fractional interval; masked_fraction_data() equals np.histogram(parsed fractions, np.arange(0, 1.0, 0.01));
  * the reads include some without qualities ("-nan"), with '!' alone ("-0.000"), one without bases, and masked fractions printed 0.290,
    0.350, 0.570, 0.990, 0.991 and 1.000: 0.350 and 0.570 lie below the np.arange edge of their name (0.35000000000000003,
    0.5700000000000001) and fall into the bin below, 0.290 does not (29 * 0.01 is 0.29 itself with numpy 2.2), 0.990 is the closed last
    edge, the last two are counted nowhere;
  * SampleQCPass.figures() is what it was, figures(per_read=True) adds "qscore" and "masked";
  * CoverageTable.length_vs_coverage_data() and qscore_data() equal the oracle on the rows of tests/golden/tiny_ava.table.gz."""
import gzip
import os
from decimal import Decimal

import numpy as np
import pytest

from longqc_amd import api, chunkpass, sdust
from longqc_amd import figdata as F
from longqc_amd.covtable import CoverageTable
from tests import test_boxstats as TB
from tests.conftest import GOLDEN
from tests.test_sdust_table import ADP3, ADP5

MISSING = F.MISSING
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
# (bases of A, length): a run of A is masked whole, the tail behind it -- a C, then random bases -- not at all
RUNS = ((29, 100), (290, 1000), (35, 100), (350, 1000), (57, 100), (570, 1000), (99, 100), (990, 1000), (991, 1000), (200, 200), (1000, 1000))
WANTED = {290, 350, 570, 990, 991, 1000}


def make_reads():
    rng = np.random.default_rng(31)

    def bases(n):
        return ACGT[rng.integers(0, 4, n)].tobytes().decode()

    def quals(n):
        return (rng.integers(2, 40, n) + 33).astype(np.uint8).tobytes().decode()
    reads = [["run%d_%d" % (k, l), "A" * k + ("C" + bases(l - k - 1) if l > k else ""), quals(l)] for k, l in RUNS]
    for i, l in enumerate(np.concatenate([rng.integers(40, 5000, 230), rng.integers(5000, 12000, 12)]).tolist()):
        q = None if i % 9 == 4 else "!" * l if i % 31 == 7 else quals(l)
        reads.append(["r%d" % i, bases(l), q])
    reads.insert(50, ["no_bases", "", None])
    return reads


def parsed_file(path):
    """-> (lengths, fractions, meanQ as thousandths or None) of the table, every field read again from its text"""
    lens, frac, qv = [], [], []
    for row in open(path).read().splitlines():
        f = row.split("\t")
        lens.append(int(f[2]))
        for t, out in ((f[3], frac), (f[4], qv)):
            out.append(None if "nan" in t else int(Decimal(t) * 1000))
            assert out[-1] is None or (len(t.split(".")[1]) == 3 and Decimal(out[-1]) == Decimal(t) * 1000)
    return np.array(lens, dtype=np.int64), frac, qv


def mask_of(reads, lib, tmp_path, table, tag, chunks=3):
    m = sdust.LqMaskMI355X(str(tmp_path / (tag + "_" + table)), lib=lib, table=table)
    per = (len(reads) + chunks - 1) // chunks
    for c in range(chunks):
        m.submit_sdust(reads[c * per:(c + 1) * per], c)
    return m


def check_mask(lib, tmp_path):
    reads = make_reads()
    host, dev = (mask_of(reads, lib, tmp_path, t, "main") for t in ("host", "device"))
    for a, b in zip(host.columns(), dev.columns()):
        assert a.dtype == b.dtype and a.tolist() == b.tolist()         # both modes, the same arrays
    host.close_pool(); dev.close_pool()
    assert open(host.get_outfile_path(), "rb").read() == open(dev.get_outfile_path(), "rb").read()
    lens, frac, qv = parsed_file(dev.get_outfile_path())
    frac_thou = np.array([0xffffffff if f is None else f for f in frac], dtype=np.uint32)
    qv_thou = np.array([MISSING if q is None else q for q in qv], dtype=np.int32)
    got = dev.columns()
    assert got[0].tolist() == lens.tolist() and got[1].tolist() == frac_thou.tolist() and got[2].tolist() == qv_thou.tolist()
    text = open(dev.get_outfile_path()).read()
    assert "\t-0.000\t" in text and "\t-nan\t-nan\t" in text and int((qv_thou == MISSING).sum()) >= 20 and int((frac_thou == 0xffffffff).sum()) == 1
    assert WANTED <= set(frac_thou.tolist()), sorted(set(frac_thou.tolist()) & set(range(250, 1001)))
    for m in (host, dev):
        # the QV box plot by length bin
        n50 = m.summary()["n50"]
        assert n50 >= 3000
        for interval, want_interval in ((None, 3000), (1234.5, 1234.5)):
            q = m.qscore_figure_data(interval)
            assert q["interval"] == want_interval and q["mid_threshold"] == 7
            TB.same_boxes(q, TB.oracle(lens, qv_thou, float(want_interval)), "QV by length bin, interval %r" % (interval,))
            assert len(q["group"]) >= 4 and int(q["n_all"].sum()) == len(reads) and int(q["n"].sum()) == len(reads) - int((qv_thou == MISSING).sum())
        assert m.qscore_figure_data(platform="rs2")["mid_threshold"] == 8
        # the masked-fraction histogram
        edges, counts = m.masked_fraction_data()
        want_edges = np.arange(0, 1.0, 0.01)
        column = np.array([np.nan if f is None else float(Decimal(f) / 1000) for f in frac])
        with np.errstate(invalid="ignore"):
            want = np.histogram(column, bins=want_edges)[0]
        assert edges.tobytes() == want_edges.tobytes() and counts.dtype == np.int64 and counts.tolist() == want.tolist()
        assert counts.sum() == len(reads) - 1 - int((frac_thou[frac_thou != 0xffffffff] > 990).sum())
        assert counts[34] >= 1 and counts[56] >= 1 and counts[98] >= 1    # 0.350 and 0.570 in the bin below their name's, 0.990 on the last edge
    assert (want_edges > np.arange(100) / 100).sum() >= 5 and want_edges[35] > 0.35 and want_edges[57] > 0.57      # edges above their k / 100
    table = F.masked_bin_table()                                     # the fold, against np.histogram itself for each of the 1001 printed values
    for k in range(1001):
        c = np.histogram(np.array([k / 1000]), bins=want_edges)[0]
        assert table[k] == (int(np.argmax(c)) if c.sum() else 99), k
    assert (table != 99).sum() == 991


def check_interval_rule_and_refusals(lib, tmp_path):
    rng = np.random.default_rng(2)
    reads = [["s%d" % i, ACGT[rng.integers(0, 4, l)].tobytes().decode(), "5" * l] for i, l in enumerate([401, 250, 1701, 1701, 900, 95, 2200, 1300])]
    m = mask_of(reads, lib, tmp_path, "device", "short", chunks=2)
    n50 = m.summary()["n50"]
    assert n50 == 1701                                               # below 3000 and odd: the interval is fractional (longQC.py:478-481)
    q = m.qscore_figure_data()
    assert q["interval"] == n50 / 2 == 850.5
    lens, _, qv = m.columns()
    TB.same_boxes(q, TB.oracle(lens, qv, 850.5), "QV by length bin, interval n50 / 2")
    assert q["group"].tolist() == [0, 1, 2] and len(q["fliers"]) == 3
    empty = sdust.LqMaskMI355X(str(tmp_path / "empty"), lib=lib)
    for call in (empty.qscore_figure_data, empty.masked_fraction_data):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        m.qscore_figure_data(interval=0)
    # the columns belong to a table: none before one, none after a new scan
    ch = sdust._chunk_of([r[0] for r in reads], [m._arr(r[1]) for r in reads], [m._arr(r[2]) for r in reads], 0, lib)
    try:
        with pytest.raises(api.LqcovError) as e:
            ch.sdust_columns()
        assert e.value.code == -4                                   # LQCOV_E_STATE
        ch.sdust_table()
        f1, q1 = ch.sdust_columns()
        assert (f1.tolist(), q1.tolist()) == tuple(a.tolist() for a in sdust.columns_of_rows(sdust.sdust_rows([r[0] for r in reads], None, None, lib=lib, chunk=ch)))
        with pytest.raises(api.LqcovError) as e:
            ch.sdust_columns()                                      # (sdust_rows scanned again: the table is the old scan's)
        assert e.value.code == -4
    finally:
        ch.close()


def check_pass_figures(lib, tmp_path):
    p = chunkpass.SampleQCPass(str(tmp_path / "run"), "ont-ligation", adp5=ADP5, adp3=ADP3, nsample=15, gc_draw="device", gc_seed=3, lib=lib)
    try:
        p.run_file(os.path.join(GOLDEN, "tiny_all.fq.gz"), chunk_size=100000, str_overhead=49)
        plain, more = p.figures(), p.figures(per_read=True)
        assert set(plain) == {"gc", "length"} and set(more) == {"gc", "length", "qscore", "masked"}
        for k in ("gc", "length"):
            assert set(plain[k]) == set(more[k])
        assert plain["length"]["hist"][2].tobytes() == more["length"]["hist"][2].tobytes() and plain["gc"]["read_kde"].tobytes() == more["gc"]["read_kde"].tobytes()
        p.mask.close_pool()
        lens, frac, qv = parsed_file(p.mask.get_outfile_path())
        assert len(lens) == 120
        interval = 3000 if p.summary()["n50"] >= 3000 else p.summary()["n50"] / 2
        TB.same_boxes(more["qscore"], TB.oracle(lens, [MISSING if q is None else q for q in qv], float(interval)), "tiny_all, QV by length bin")
        assert more["masked"][1].tolist() == np.histogram(np.array([f / 1000 for f in frac]), bins=np.arange(0, 1.0, 0.01))[0].tolist()
    finally:
        p.close()


def check_coverage_table(lib, tmp_path):
    t = tmp_path / "tiny_ava.table"
    t.write_bytes(gzip.open(os.path.join(GOLDEN, "tiny_ava.table.gz")).read())
    ct = CoverageTable(str(t))
    rows = [l.split("\t") for l in open(str(t)).read().splitlines()]
    thou = lambda c: np.array([MISSING if "nan" in r[c] else int(Decimal(r[c]) * 1000) for r in rows], dtype=np.int64)
    qlen, t1, qv, cov = np.array([int(r[1]) for r in rows]), thou(5), thou(6), thou(8)
    assert any(r[8] == "0.0" for r in rows) and (qlen >= 3000).sum() >= 10 and (qlen < 3000).sum() >= 10 and (t1 != cov).any()
    for c, want in ((5, t1), (6, qv), (8, cov)):
        assert ct.thousandths(c).tolist() == want.tolist() and (ct.thousandths(c) / 1000).tolist() == [float(r[c]) for r in rows]
    for interval in (3000.0, 1000.0):
        d = ct.length_vs_coverage_data(interval, lib=lib)
        TB.same_boxes(d["boxes"], TB.oracle(qlen, np.where(qlen >= 3000, cov, t1), interval), "MERGED_COVERAGE by length bin")
        by_cov = TB.oracle(qlen, cov, interval)
        assert d["group"].tolist() == [b["group"] for b in by_cov] and d["median"].tolist() == [b["median"] for b in by_cov]
        assert d["size"].tolist() == [b["n_all"] for b in by_cov] and d["reliable"].tolist() == [b["n_all"] >= 100 for b in by_cov]
        assert len(by_cov) >= 3
    q = ct.qscore_data(lib=lib)
    TB.same_boxes(q, TB.oracle((cov != 0).astype(np.int64), qv), "QV by coverage zero or not")
    assert q["group"].tolist() == [0, 1] and q["n_all"].tolist() == [int((cov == 0).sum()), int((cov != 0).sum())]
    assert CoverageTable._thou("0.0") == 0 and CoverageTable._thou("-nan") == MISSING and CoverageTable._thou("-0.000") == 0 and CoverageTable._thou("12.345") == 12345
    with pytest.raises(ValueError):
        CoverageTable._thou("1e3")


def test_emulated_mask_columns_and_figures(emu_lib, tmp_path):
    check_mask(emu_lib, tmp_path)


def test_emulated_interval_rule_and_refusals(emu_lib, tmp_path):
    check_interval_rule_and_refusals(emu_lib, tmp_path)


def test_emulated_pass_figures(emu_lib, tmp_path):
    check_pass_figures(emu_lib, tmp_path)


def test_emulated_coverage_table_boxes(emu_lib, tmp_path):
    check_coverage_table(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_mask_columns_and_figures(gpu_lib, tmp_path):
    check_mask(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_interval_rule_and_refusals(gpu_lib, tmp_path):
    check_interval_rule_and_refusals(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_pass_figures(gpu_lib, tmp_path):
    check_pass_figures(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_coverage_table_boxes(gpu_lib, tmp_path):
    check_coverage_table(gpu_lib, tmp_path)

"""longqc_amd.rs.run_platformqc end to end against what the reference's own lq_rs.run_platformqc wrote for the same run directories
(tests/golden/rs/ and tests/golden/rs.json, make_rs_golden.py), under the wave emulator and on the GPU.  Integers, the mean and N50 / N90
are exact (the sums lie far below 2^53); the gamma parameters within rel 1e-9, the bound tests/test_figdata_gamma.py uses against scipy;
Mean_HQ_fraction within n * 2^-52 * mean|fraction|, the bound tests/test_sequel_platformqc.py uses; histogram counts exact and densities
bit for bit; the box statistics by Interval equal matplotlib.cbook.boxplot_stats' recorded doubles."""
import json
import os
import shutil

import numpy as np
import pytest

from longqc_amd import api, rs
from tests.conftest import GOLDEN

GOLD = json.load(open(os.path.join(GOLDEN, "rs.json")))
RUN_DIR = os.path.join(GOLDEN, "rs")
XML = open(os.path.join(RUN_DIR, "lf", "m.sts.xml")).read()


def check_box(got, want, what):
    assert got["group"].tolist() == [b["group"] for b in want] and got["n"].tolist() == [b["n"] for b in want], what
    for k in ("q1", "med", "q3", "whislo", "whishi", "median"):
        assert got[k].tolist() == [b[k] for b in want], (what, k)
    for f, b in zip(got["fliers"], want):
        assert sorted(f.tolist()) == sorted(b["fliers"]), (what, b["group"])


def check_run(lib, run, tmp_path):
    want = GOLD["runs"][run]
    out = str(tmp_path / ("out_" + run))
    js, fig = rs.run_platformqc(os.path.join(RUN_DIR, run), out, suffix="t1", lib=lib)
    wj = want["json"]
    assert list(js) == list(wj)                                         # the reference's keys, in its order
    assert js["Productivity"] == wj["Productivity"] == dict(zip(("P0", "P1", "P2"), want["productivity"]))
    for key in ("Throughput", "Longest_read", "Num_of_reads"):
        assert type(js[key]) is int and js[key] == wj[key], key
    assert wj["Throughput"] < 2 ** 53 // 100
    for key in ("Mean_polread_length", "N50_polread_length"):
        assert type(js[key]) is float and js[key] == wj[key], key
    assert fig["n50"] == wj["N50_polread_length"] and fig["n90"] == want["N90"] and fig["mean"] == wj["Mean_polread_length"]
    a, b = js["polread_gamma_params"]
    print("%s: gamma (%r, %r) against scipy's %r" % (run, a, b, wj["polread_gamma_params"]))
    assert (a, b) == pytest.approx(tuple(wj["polread_gamma_params"]), rel=1e-9) and (fig["gamma_a"], fig["gamma_b"]) == (a, b)
    n = wj["Num_of_reads"]
    bound = n * 2.0 ** -52 * want["mean_abs_fraction"]
    print("%s: Mean_HQ_fraction %r against %r, bound %.3g" % (run, js["Mean_HQ_fraction"], wj["Mean_HQ_fraction"], bound))
    assert type(js["Mean_HQ_fraction"]) is float and abs(js["Mean_HQ_fraction"] - wj["Mean_HQ_fraction"]) <= bound
    for key in ("hq", "bases"):
        h = want["hist"][key]
        assert fig[key + "_edges"].tolist() == h["edges"] and fig[key + "_counts"].tolist() == h["counts"], (run, key)
        assert np.array_equal(fig[key + "_density"].view(np.uint64), np.array(h["density"]).view(np.uint64)), (run, key)
        assert int(fig[key + "_counts"].sum()) == n
    check_box(fig["box"], want["box"], run)
    assert json.load(open(os.path.join(out, "QC_vals_rs_t1.json"))) == js
    st = fig["stats"]
    assert st["rows"] == len(want["columns"]["NumBases"]["values"]) and st["fields_device"] == 4 * st["rows"] and st["fields_host"] == 0, st


def check_golden_runs(lib, tmp_path):
    for run in GOLD["runs"]:
        check_run(lib, run, tmp_path)
    # the golden boxes hold the groups the issue names: one of a single row, one whose values are all equal
    box = GOLD["runs"]["lf"]["box"]
    assert any(b["n"] == 1 for b in box) and any(b["n"] > 1 and b["whislo"] == b["whishi"] for b in box)


def run_dir(tmp_path, name, csv, xml=XML):
    d = tmp_path / name
    d.mkdir()
    if csv is not None:
        (d / "m1.sts.csv").write_bytes(csv)
    if xml is not None:
        (d / "m1.sts.xml").write_text(xml)
    return str(d)


HEAD = b"ReadScore,HQRegionStart,HQRegionEnd,NumBases\n"


def check_errors(lib, tmp_path):
    rows = b"0.8,0,1500,1600\n0.9,10,2510,2600\n0.05,0,0,40\n0.7,5,3005,3100\n"
    js, fig = rs.run_platformqc(run_dir(tmp_path, "noxml", HEAD + rows, xml=None), lib=lib)        # a missing sts.xml
    assert js["Productivity"] == {"P0": None, "P1": None, "P2": None} and js["Num_of_reads"] == 3 and js["Throughput"] == 7000
    assert not os.path.exists(str(tmp_path / "noxml" / "QC_vals_rs.json"))
    with pytest.raises(FileNotFoundError, match="csv"):                 # a missing sts.csv
        rs.run_platformqc(run_dir(tmp_path, "nocsv", None), lib=lib)
    with pytest.raises(FileNotFoundError):
        rs.run_platformqc(str(tmp_path / "nowhere"), lib=lib)
    with pytest.raises(api.LqcovError) as e:                            # a negative HQ length, in a row the mask leaves out as well
        rs.run_platformqc(run_dir(tmp_path, "negative", HEAD + rows + b"0.01,700,699,800\n"), lib=lib)
    assert e.value.code == -5 and "1 rows" in str(e.value) and "below 0" in str(e.value)
    with pytest.raises(api.LqcovError) as e:                            # ... and one above 2^32-1
        rs.run_platformqc(run_dir(tmp_path, "huge", HEAD + rows + b"0.9,0,4294967296,4294967297\n"), lib=lib)
    assert e.value.code == -5
    with pytest.raises(ValueError, match="empty"):                      # no row above 0.1: the reference's max() of an empty array
        rs.run_platformqc(run_dir(tmp_path, "none", HEAD + b"0.1,0,1500,1600\n0.10,10,2510,2600\n0.05,0,0,40\n"), lib=lib)
    with pytest.raises(ValueError, match="length of 0"):                # an HQ region of length 0 under the mask: scipy's fit raises
        rs.run_platformqc(run_dir(tmp_path, "zero", HEAD + rows + b"0.9,50,50,80\n"), lib=lib)
    with pytest.raises(api.LqcovError) as e:                            # the table's own errors come with the file and the line
        rs.run_platformqc(run_dir(tmp_path, "ragged", HEAD + rows + b"0.9,50\n"), lib=lib)
    assert e.value.code == -5 and "m1.sts.csv" in str(e.value) and "line 6: " in str(e.value)
    with pytest.raises(api.LqcovError, match="no column 'NumBases'"):
        rs.run_platformqc(run_dir(tmp_path, "nocol", b"ReadScore,HQRegionStart,HQRegionEnd\n0.8,0,1500\n"), lib=lib)


def test_host_parts(tmp_path):
    p = tmp_path / "m.sts.xml"
    p.write_text(XML)
    assert rs.parse_sts_xml(str(p)) == GOLD["runs"]["lf"]["productivity"]
    p.write_text(XML.replace(">Other<", ">Another Productive Other<").replace(">Undefined<", ">Empty again<"))
    assert rs.parse_sts_xml(str(p)) == [0, 7, 0]                        # the first of Empty, Productive, Other a label contains; of two bins with one label the later
    p.write_text(XML.replace("PipelineStats/PipeStats.xsd", "PacBioPipelineStats.xsd"))
    assert rs.parse_sts_xml(str(p)) == [0, 0, 0]                        # another namespace: nothing found, the defaults
    assert rs.get_sts_xml_path(str(tmp_path)) == str(p) and rs.get_sts_csv_path(str(tmp_path)) is None
    assert rs.get_sts_xml_path(str(tmp_path / "none")) is None and rs.get_sts_csv_path(str(tmp_path / "none")) is None
    shutil.copy(os.path.join(RUN_DIR, "crlf", "m.sts.csv"), str(tmp_path / "a.sts.csv"))
    assert rs.get_sts_csv_path(str(tmp_path)) == str(tmp_path / "a.sts.csv")


def test_emulated_platformqc_equals_the_reference(emu_lib, tmp_path):
    check_golden_runs(emu_lib, tmp_path)


def test_emulated_platformqc_errors(emu_lib, tmp_path):
    check_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_platformqc_equals_the_reference(gpu_lib, tmp_path):
    check_golden_runs(gpu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_platformqc_errors(gpu_lib, tmp_path):
    check_errors(gpu_lib, tmp_path)

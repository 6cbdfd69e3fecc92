"""longqc_amd.sequel.run_platformqc end to end against what the reference's own functions gave for the same records
(tests/golden/polread.json, runs): two small BAMs and an sts.xml are written from the golden record lists with tests/bam_writer.py, and the
JSON block, the figure data and the errors are compared -- from every byte path: host inflate, device inflate, device inflate with the
inflated bytes kept on the device, and pieces so small that records and ZMWs straddle them.  Under the wave emulator and on the GPU."""
import gc
import json
import os
import warnings

import numpy as np
import pytest

from longqc_amd import api, sequel
from tests import bam_writer as BW
from tests import polread_cases
from tests.test_polread_fields import IP, RG, SN, tag_a

GOLD = polread_cases.load()
RUNS = {r["name"]: r for r in GOLD["runs"]}
HEADER = "@HD\tVN:1.5\tSO:unknown\tpb:3.0.1\n@RG\tID:a1b2c3d4\tPL:PACBIO\tDS:READTYPE=%s;Ipd:CodecV1=ip;BINDINGKIT=100;SEQUENCINGKIT=101\tPU:m54_1\n@PG\tID:baz2bam\n"
STS = """<?xml version="1.0" encoding="utf-8"?>
<PipeStats xmlns="http://pacificbiosciences.com/PacBioPipelineStats.xsd" xmlns:ns="http://pacificbiosciences.com/PacBioBaseDataModel.xsd">
  <NumSequencingZmws>1014</NumSequencingZmws>
  <ProdDist>
    <ns:NumBins>4</ns:NumBins>
    <ns:BinCounts><ns:BinCount>301</ns:BinCount><ns:BinCount>622</ns:BinCount><ns:BinCount>91</ns:BinCount><ns:BinCount>0</ns:BinCount></ns:BinCounts>
    <ns:MetricDescription>Productivity</ns:MetricDescription>
    <ns:BinLabels><ns:BinLabel>Empty</ns:BinLabel><ns:BinLabel>Productive</ns:BinLabel><ns:BinLabel>Other</ns:BinLabel><ns:BinLabel>Undefined</ns:BinLabel></ns:BinLabels>
  </ProdDist>
</PipeStats>
"""
BASES = b"ACGT" * 8


def write_run(d, run, sts=True, block_payload=65280, scraps_type="SCRAP", subreads_type="SUBREAD"):
    os.makedirs(d, exist_ok=True)
    scraps = []
    for k, (name, sz, sc) in enumerate(run["scraps"]):
        tags = [t for t in (tag_a(b"sz", sz) if sz else None, tag_a(b"sc", sc) if sc else None, RG, SN if k % 3 else None, IP if k % 97 == 5 else None) if t]
        tags = tags[k % len(tags):] + tags[:k % len(tags)]             # sz and sc in every place and order
        scraps.append((name.encode(), BASES[:k % 30], b"".join(tags)))
    subreads = [(n[0].encode(), BASES[:k % 31], RG + SN) for k, n in enumerate(run["subreads"])]
    for path, recs, rt in (("m54_1.scraps.bam", scraps, scraps_type), ("m54_1.subreads.bam", subreads, subreads_type)):
        BW.write_bam(os.path.join(d, path), [(n, s) for n, s, _ in recs], tags=[t for _, _, t in recs], header_text=(HEADER % rt).encode(),
                     block_payload=block_payload, level=1)
    if sts:
        open(os.path.join(d, "m54_1.sts.xml"), "w").write(STS)
    return d


def check_against_golden(js, fig, want, productivity=(301, 622, 91)):
    assert js["Productivity"] == dict(zip(("P0", "P1", "P2"), productivity))
    for key in ("Throughput", "Longest_read", "Num_of_reads"):
        assert type(js[key]) is int and js[key] == want[key], key
    assert type(js["Throughput(Control)"]) is int and js["Throughput(Control)"] == want["control"]
    for key in ("Mean_polread_length", "N50_polread_length"):
        assert type(js[key]) is float and js[key] == want[key], key  # integer sums below 2^53: exact in any order
    assert fig["n50"] == want["N50_polread_length"] and fig["n90"] == want["N90"] and fig["mean"] == want["Mean_polread_length"]
    assert js["Adapter_observation"] == {int(k): v for k, v in want["Adapter_observation"].items()}
    n = want["Num_of_reads"]
    print("Mean_HQ_fraction %r against %r, bound %.3g" % (js["Mean_HQ_fraction"], want["Mean_HQ_fraction"], n * 2.0 ** -52 * want["mean_abs_fraction"]))
    assert abs(js["Mean_HQ_fraction"] - want["Mean_HQ_fraction"]) <= n * 2.0 ** -52 * want["mean_abs_fraction"]
    a, b = js["polread_gamma_params"]
    print("gamma (%r, %r) against scipy's %r" % (a, b, want["gamma"]))
    assert (a, b) == pytest.approx(tuple(want["gamma"]), rel=1e-9)    # tests/test_figdata_gamma.py's bound for gamma_fit against scipy
    assert (fig["gamma_a"], fig["gamma_b"]) == (a, b)
    hr, tot = fig["hr_lengths"], fig["tot_lengths"]
    assert hr.size == n and int(hr.min()) == want["min_hr"] and (int(tot.min()), int(tot.max())) == (want["min_tot"], want["max_tot"])
    for key, x in (("hr", hr), ("tot", tot)):
        edges = np.arange(x.min(), x.max() + 1000, 1000)
        density, e = np.histogram(x, bins=edges, density=True)
        assert np.array_equal(fig[key + "_edges"], e) and np.array_equal(fig[key + "_density"], density) and fig[key + "_counts"].sum() == n
    lo, hi = min(js["Adapter_observation"]), max(js["Adapter_observation"])
    assert fig["adapter_left"] == list(range(lo, hi + 1)) and fig["adapter_height"] == [js["Adapter_observation"].get(i, 0) for i in range(lo, hi + 1)]


def check_paths(lib, tmp_path, monkeypatch):
    run = RUNS["main"]
    d = write_run(str(tmp_path / "run"), run)
    n_rec = len(run["scraps"]) + len(run["subreads"])
    out = str(tmp_path / "out")
    js, fig = sequel.run_platformqc(d, out, suffix="x1", inflate="host", lib=lib)
    check_against_golden(js, fig, run["expect"])
    assert json.load(open(os.path.join(out, "QC_vals_sequel_x1.json"))) == json.loads(json.dumps(js))
    assert fig["stats"]["records_device"] == n_rec and fig["stats"]["records_host"] == fig["stats"]["records_flagged"] == 0
    first = json.dumps(js, sort_keys=True)
    for inflate, host_copy in (("device", "all"), ("device", "needed")):
        js2, fig2 = sequel.run_platformqc(d, inflate=inflate, host_copy=host_copy, lib=lib)
        assert json.dumps(js2, sort_keys=True) == first
        st = fig2["stats"]
        assert st["records_device"] == n_rec and st["bytes_inflated"] == fig["stats"]["bytes_inflated"]
        if host_copy == "needed":                                       # the headers, and nothing else, came to the host
            assert 0 < st["bytes_to_host"] < 2 * (len(HEADER) + 64), st
        else:
            assert st["bytes_to_host"] == st["bytes_inflated"]
    # pieces shorter than a ZMW's records, in BGZF blocks shorter than a piece: records straddle both
    d2 = write_run(str(tmp_path / "run2"), run, block_payload=701)
    monkeypatch.setenv("LQPOL_PIECE_BYTES", "3000")
    for inflate, host_copy in (("host", "all"), ("device", "needed")):
        js3, fig3 = sequel.run_platformqc(d2, inflate=inflate, host_copy=host_copy, lib=lib)
        assert json.dumps(js3, sort_keys=True) == first and fig3["stats"]["pieces"] > 50
        assert fig3["stats"]["records_device"] + fig3["stats"]["records_host"] == n_rec
    monkeypatch.delenv("LQPOL_PIECE_BYTES")
    # the per-ZMW results of the small run, every ZMW of the reference's dict
    small = RUNS["small"]
    d3 = write_run(str(tmp_path / "run3"), small, sts=False)
    with sequel.PolymeraseReads(lib=lib) as p:
        p.add_scraps(os.path.join(d3, "m54_1.scraps.bam"))
        p.add_subreads(os.path.join(d3, "m54_1.subreads.bam"))
        p.finish()
        got = {str(z): [int(h), int(t), bool(i), int(a)] for z, h, t, i, a in zip(p.all_zmw, p.all_hq, p.all_tot, p.is_pol, p.all_ad_num)}
        assert got == small["expect"]["per_zmw"]
        check_against_golden(p.json_block(), p.figure_data(), small["expect"], (None, None, None))


def check_errors(lib, tmp_path):
    small = RUNS["small"]
    d = write_run(str(tmp_path / "run"), small, sts=False)
    js, _ = sequel.run_platformqc(d, lib=lib)
    assert js["Productivity"] == {"P0": None, "P1": None, "P2": None}    # a missing sts.xml
    scraps, subreads = os.path.join(d, "m54_1.scraps.bam"), os.path.join(d, "m54_1.subreads.bam")
    with sequel.PolymeraseReads(lib=lib) as p:                           # subreads before scraps
        p.add_subreads(subreads)
        with pytest.raises(api.LqcovError) as e:
            p.add_scraps(scraps)
        assert e.value.code == -4 and "scraps after subreads" in str(e.value)
    for kw in ({"scraps_type": "SUBREAD"}, {"subreads_type": "CCS"}):   # a wrong READTYPE
        with pytest.raises(ValueError, match="READTYPE"):
            sequel.run_platformqc(write_run(str(tmp_path / ("wrong_" + list(kw)[0])), small, **kw), lib=lib)
    with sequel.PolymeraseReads(lib=lib) as p:                           # ... is refused before the file is read: nothing of it is in the handle
        with pytest.raises(ValueError, match="READTYPE"):
            p.add_scraps(subreads)                                        # (a subreads file given as the scraps file)
        p.finish()
        assert len(p.all_zmw) == 0 and p.stats["pieces"] == 0
    assert sequel.get_readtype(sequel.file_header(scraps, lib)) == "SCRAP" and sequel.file_header(subreads, lib) == (HEADER % "SUBREAD").encode()
    # a polymerase read with tot == 0: finish() raises as the reference's hq / tot does, and so does what needs the fractions afterwards
    with sequel.PolymeraseReads(lib=lib) as p:
        p.add_items([1, 1, 2], [100, 50, 0], [50, 10, 9], "SAS")
        for call in (p.finish, p.json_block, p.figure_data):
            with pytest.raises(ZeroDivisionError):
                call()
        assert p.all_tot.tolist() == [0, 10]
    # a constructor that fails leaves nothing for __del__ to trip over
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="inflate"):
            sequel.PolymeraseReads(inflate="elsewhere", lib=lib)
        gc.collect()
    # a truncated file: cut inside a BGZF block, and at a block's end inside a record
    raw = open(scraps, "rb").read()
    whole = BW.bam_stream([(b"m/1/0_5", b"ACGT")] * 40, header_text=(HEADER % "SCRAP").encode())
    for name, content, what in (("cut_block", raw[:len(raw) // 2], "BGZF block"), ("cut_record", BW.bgzf(whole[:-7]), "the file ends inside a record")):
        dd = str(tmp_path / name)
        os.makedirs(dd)
        open(os.path.join(dd, "m.scraps.bam"), "wb").write(content)
        open(os.path.join(dd, "m.subreads.bam"), "wb").write(open(subreads, "rb").read())
        for inflate in ("host", "device"):
            with pytest.raises(api.LqcovError) as e:
                sequel.run_platformqc(dd, inflate=inflate, lib=lib)
            assert e.value.code == -2 and what in str(e.value) and "m.scraps.bam" in str(e.value), str(e.value)
    # a directory without one of the two BAMs
    dd = str(tmp_path / "half")
    os.makedirs(dd)
    open(os.path.join(dd, "m.subreads.bam"), "wb").write(open(subreads, "rb").read())
    with pytest.raises(FileNotFoundError, match="scraps"):
        sequel.run_platformqc(dd, lib=lib)
    with pytest.raises(FileNotFoundError):
        sequel.run_platformqc(str(tmp_path / "nowhere"), lib=lib)
    # a polymerase read of HQ length 0: scipy's fit raises (a ValueError) inside the reference, and so does this one
    zero = RUNS["zero_hq"]
    assert GOLD["zero_hq"]["mro"][1] == "ValueError" and zero["expect"]["gamma_error"]["mro"][1] == "ValueError" and zero["expect"]["min_hr"] == 0
    with pytest.raises(ValueError, match="HQ length of 0"):
        sequel.run_platformqc(write_run(str(tmp_path / "zero"), zero), lib=lib)


def test_host_parts():
    assert sequel.get_readtype(HEADER % "SCRAP") == "SCRAP" and sequel.get_readtype((HEADER % "SUBREAD").encode()) == "SUBREAD"
    assert sequel.get_readtype("@HD\tVN:1.5\n@RG\tID:x\tDS:BINDINGKIT=1\n") is None and sequel.get_readtype("") is None
    assert sequel.get_readtype("@RG\tID:x\tDS:a=b\n@RG\tID:y\tDS:Q=1;READTYPE=CCS\n") == "CCS"
    assert sequel.get_readtype("@RG\tDS:xREADTYPE=1;READTYPE=A=B;READTYPE=C\tID:y\r\n") == "A"      # the first entry whose key is READTYPE, up to a second '='
    assert sequel.get_readtype("@CO\tDS:READTYPE=NO\n@RG\tID:y\tDS:READTYPE=FIRST\tDS:READTYPE=LAST\n") == "LAST"      # (a repeated field: the last, as in a dict)


def test_sts_xml(tmp_path):
    p = tmp_path / "m.sts.xml"
    p.write_text(STS)
    assert sequel.parse_sts_xml(str(p)) == [301, 622, 91]
    p.write_text(STS.replace(">Other<", ">Another Productive Other<").replace(">Undefined<", ">Empty again<"))
    assert sequel.parse_sts_xml(str(p)) == [0, 91, 0]                  # the first of Empty, Productive, Other a label contains; of two bins with one label the later
    p.write_text(STS)
    assert sequel.get_sts_xml_path(str(tmp_path)) == str(p) and sequel.get_sts_xml_path(str(tmp_path / "none")) is None


def test_emulated_platformqc_equals_the_reference(emu_lib, tmp_path, monkeypatch):
    check_paths(emu_lib, tmp_path, monkeypatch)


def test_emulated_platformqc_errors(emu_lib, tmp_path):
    check_errors(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_platformqc_equals_the_reference(gpu_lib, tmp_path, monkeypatch):
    check_paths(gpu_lib, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_platformqc_errors(gpu_lib, tmp_path):
    check_errors(gpu_lib, tmp_path)

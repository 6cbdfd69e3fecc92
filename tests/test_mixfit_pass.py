"""SampleQCPass.coverage_stats(): the Coverage_stats block of the run's JSON from the table coverage() made, on the smallest synthetic
dataset of the pass tests (tests/golden/tiny_all.fq.gz).  It equals CoverageTable(the file coverage() wrote).est_coverage().json_block(the
pass's own yield), and asking for it before coverage() is an error."""
import os

import pytest

from longqc_amd import chunkpass
from longqc_amd.covtable import CoverageTable
from tests.conftest import GOLDEN


def check_pass_stats(lib, tmp_path):
    p = chunkpass.SampleQCPass(str(tmp_path / "run"), "ont-ligation", nsample=60, gc_draw="device", gc_seed=3, lib=lib)
    try:
        p.run_file(os.path.join(GOLDEN, "tiny_all.fq.gz"), chunk_size=100000, str_overhead=49)
        with pytest.raises(RuntimeError):
            p.coverage_stats()
        out = str(tmp_path / "coverage_out.txt")
        p.coverage(out=out)
        got = p.coverage_stats()
        t = CoverageTable(out).est_coverage(lib=lib)
        assert p.n_bases > 0 and got == t.json_block(p.n_bases)
        assert got["Estimated crude Xome size"] == t.calc_xome_size(p.n_bases) and got["Estimated non-sense read fraction"] == t.get_unmapped_med_frac()
        assert ("Mean_coverage" in got) != ("Mode_coverage" in got)
        assert p.coverage_table.model["n_iter"] == t.model["n_iter"] and p.coverage_table.get_mean() == t.get_mean()
        rna = p.coverage_stats(is_transcript=True)
        assert set(rna) == {"Estimated non-sense read fraction", "Mode_coverage", "mu_coverage", "sigma_coverage", "Estimated crude Xome size"}
        assert rna["Mode_coverage"] == float(CoverageTable(out).est_coverage(True, lib=lib).get_logn_mode())
    finally:
        p.close()


def test_emulated_pass_coverage_stats(emu_lib, tmp_path):
    check_pass_stats(emu_lib, tmp_path)


@pytest.mark.gpu
def test_gpu_pass_coverage_stats(gpu_lib, tmp_path):
    check_pass_stats(gpu_lib, tmp_path)

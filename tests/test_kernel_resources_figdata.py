"""Registers, spills and LDS of the figure-data kernels (kernels_figdata.hpp, hipcc's resource remarks, no GPU).  None may spill or take
AGPRs.  k_fig_hist's LDS is the edges and the block-private counters of LQ_FIG_HIST_LDS_BINS bins and nothing else, (bins + 1) x 8 + bins x
4 bytes, in the 16-byte granules the remark reports; the others use none.  The bounds are the VGPR step of the occupancy table that the
first clean build lands on, 8 waves per SIMD up to 64 VGPRs: k_fig_kde 50 (the double-precision exp inlined, one accumulator per lane),
k_fig_logsum 49 (log), k_fig_fold 31 (eight partials in flight), k_fig_hist 17 for both element types, k_fig_range 8."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import test_launch_caps as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["k_fig_range", "k_fig_hist<float>", "k_fig_hist<unsigned int>", "k_fig_kde", "k_fig_logsum", "k_fig_fold"]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "figdata.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert set(KERNELS) <= set(rows), r.stdout[-2000:]
    return rows


@pytest.mark.parametrize("kernel", KERNELS)
def test_figure_kernels_use_no_scratch_and_no_agprs(resources, kernel):
    r = resources[kernel]
    assert r["scratch"] == 0 and r["agpr"] == 0, r


@pytest.mark.parametrize("kernel", KERNELS)
def test_figure_kernels_keep_full_occupancy(resources, kernel):
    r = resources[kernel]
    assert r["vgpr"] <= 64 and r["occ"] == 8, r


def test_histogram_lds_is_the_edges_and_counters_of_its_bins(resources):
    bins = LC.header_define("LQ_FIG_HIST_LDS_BINS")
    want = ((bins + 1) * 8 + bins * 4 + 15) // 16 * 16
    for name in KERNELS:
        assert resources[name]["lds"] == (want if name.startswith("k_fig_hist") else 0), (name, resources[name], want)

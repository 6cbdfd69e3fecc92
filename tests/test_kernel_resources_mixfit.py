"""Registers, spills and LDS of the two mixture-fit kernels (kernels_mixfit.hpp), from hipcc's resource remarks, no GPU.  Neither may spill or
take AGPRs.  LDS is what the header states: k_mix_gmm2 the segment, LQ_MIX_MAX_N doubles = 73728 bytes (two blocks per CU); k_mix_lognorm
the segment, its logarithms and the LQ_MIX_MAX_TOL_ITERS log-likelihoods of mixem's stopping rule = 147968 bytes (one block per CU).  The
VGPR bound is the occupancy step the first clean build lands on, 4 waves per SIMD up to 128 VGPRs (k_mix_gmm2 115: two components'
parameters and their derived numbers in doubles, five running sums; k_mix_lognorm 104); a block is one wave and LDS admits one or two
blocks per CU, so registers do not limit what runs."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import test_launch_caps as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
MAX_N, TOL_ITERS = LC.header_define("LQ_MIX_MAX_N"), LC.header_define("LQ_MIX_MAX_TOL_ITERS")
LDS = {"k_mix_gmm2": MAX_N * 8, "k_mix_lognorm": 2 * MAX_N * 8 + TOL_ITERS * 8}


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "mixfit.cpp"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert set(LDS) <= set(rows), sorted(rows)
    return rows


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_mix_kernels_use_no_scratch_and_no_agprs(resources, kernel):
    r = resources[kernel]
    assert r["scratch"] == 0 and r["agpr"] == 0, r


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_mix_kernels_lds_is_what_the_header_states(resources, kernel):
    assert resources[kernel]["lds"] == LDS[kernel] and LDS[kernel] <= 160 * 1024, resources[kernel]
    assert LDS["k_mix_gmm2"] * 2 <= 160 * 1024


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_mix_kernels_stay_within_128_vgprs(resources, kernel):
    assert resources[kernel]["vgpr"] <= 128, resources[kernel]

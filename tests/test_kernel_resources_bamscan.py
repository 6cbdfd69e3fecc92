"""Registers, spills and LDS of the BAM record walk's kernels (kernels_bamscan.hpp, hipcc's resource remarks, no GPU), after
tests/test_kernel_resources_fxscan.py.  k_bam_candidates is a streaming pass: no scratch, no LDS beyond the block scan's word per wave,
and inside the 8-wave step of the occupancy table (up to 64 VGPRs).  k_bam_link and k_bam_emit are held to what their first clean
build reached: 8 waves, 30 and 50 VGPRs."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_bam_candidates", "k_bam_link", "k_bam_emit")


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "reader.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    for k in KERNELS:
        assert k in rows, r.stdout[-2000:]
    return rows


def test_walk_kernels_use_no_scratch_and_no_agprs(resources):
    for k in KERNELS:
        print(k, resources[k])
        assert resources[k]["scratch"] == 0 and resources[k]["agpr"] == 0, (k, resources[k])


def test_the_candidate_pass_keeps_full_occupancy(resources):
    r = resources["k_bam_candidates"]
    assert r["vgpr"] <= 64 and r["occ"] == 8 and r["lds"] <= 32, r      # 64 is the 8-wave step; 32 bytes: the block scan


def test_the_other_walk_kernels_keep_their_first_build_s_occupancy(resources):
    assert resources["k_bam_link"]["occ"] == 8 and resources["k_bam_link"]["lds"] == 0, resources["k_bam_link"]
    assert resources["k_bam_emit"]["occ"] == 8 and resources["k_bam_emit"]["lds"] <= 32, resources["k_bam_emit"]

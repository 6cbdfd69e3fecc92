"""Registers, spills and LDS of the BAM reader's kernels (kernels_bam.hpp, hipcc's resource remarks, no GPU).  k_bam_gather reads
0.5 B and writes 1 B per base without LDS, and k_bam_qual is a byte gather: what hides their load latency is waves per SIMD, so both
stay without scratch and inside the 8-wave step of the occupancy table (up to 64 VGPRs), as k_chunk_gather does
(tests/test_kernel_resources_gather.py); the counts of the first clean build are recorded in DESIGN.md 8 (9)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_bam_gather", "k_bam_qual")


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "chunk.cpp"], stdout=subprocess.PIPE,
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


@pytest.mark.parametrize("kernel", KERNELS)
def test_bam_kernels_use_no_scratch_no_lds_and_no_agprs(resources, kernel):
    r = resources[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r["lds"] == 0 and r["agpr"] == 0, r


@pytest.mark.parametrize("kernel", KERNELS)
def test_bam_kernels_keep_full_occupancy(resources, kernel):
    r = resources[kernel]
    assert r["vgpr"] <= 64 and r["occ"] == 8, r                     # 64 is the 8-wave step

"""Registers, spills and LDS of the FASTQ writer's kernel (kernels_fastq.hpp, hipcc's resource remarks, no GPU).  k_fastq_format is a
streaming copy without LDS, k_chunk_gather run backwards: what hides its load latency is waves per SIMD, so it must stay without
scratch and inside the 8-wave step of the occupancy table (up to 64 VGPRs); the count of the first clean build is recorded in
DESIGN.md 8 (12)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "writer.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert "k_fastq_format" in rows, r.stdout[-2000:]
    return rows


def test_format_kernel_uses_no_scratch_no_lds_and_no_agprs(resources):
    r = resources["k_fastq_format"]
    print("k_fastq_format:", r)
    assert r["scratch"] == 0 and r["lds"] == 0 and r["agpr"] == 0, r


def test_format_kernel_keeps_full_occupancy(resources):
    r = resources["k_fastq_format"]
    assert r["vgpr"] <= 64 and r["occ"] == 8, r                     # 64 is the 8-wave step

"""Registers, spills and LDS of the record scan's kernels (kernels_fxscan.hpp, hipcc's resource remarks, no GPU).  k_fx_lines and k_fx_emit
are streaming passes: no scratch, no LDS beyond the block scan's word per wave, and inside the 8-wave step of the occupancy table (up
to 64 VGPRs), the bar k_chunk_gather and k_fastq_format are held to.  The other kernels are held to the step their first clean build
reached: 8 waves."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_fx_lines", "k_fx_tilescan", "k_fx_candidates", "k_fx_jump", "k_fx_emit", "k_fx_rebase", "k_fx_tileseg")


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


def test_scan_kernels_use_no_scratch_and_no_agprs(resources):
    for k in KERNELS:
        print(k, resources[k])
        assert resources[k]["scratch"] == 0 and resources[k]["agpr"] == 0, (k, resources[k])


def test_streaming_scan_kernels_keep_full_occupancy(resources):
    for k in ("k_fx_lines", "k_fx_emit"):
        r = resources[k]
        assert r["vgpr"] <= 64 and r["occ"] == 8 and r["lds"] <= 32, (k, r)      # 64 is the 8-wave step; 32 bytes: the block scan


def test_the_other_scan_kernels_keep_their_first_build_s_occupancy(resources):
    for k in ("k_fx_tilescan", "k_fx_candidates", "k_fx_jump", "k_fx_rebase", "k_fx_tileseg"):
        assert resources[k]["occ"] == 8 and resources[k]["lds"] <= 32, (k, resources[k])

"""Registers, spills and LDS of the table's kernels (kernels_dust_table.hpp, hipcc's resource remarks, no GPU).  The three kernels build
their digits in registers: none may use scratch, LDS or AGPRs.  k_sdust_rows carries the double-precision log10 and two exact roundings
per row; the first clean build gave it 68 VGPRs, the 7-wave step of the occupancy table (up to 72).  k_sdust_patch (19) and k_sdust_text
(28) are streaming kernels and stay inside the 8-wave step (up to 64).  The counts are recorded in DESIGN.md 8 (16)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_sdust_rows", "k_sdust_patch", "k_sdust_text")
BOUNDS = {"k_sdust_rows": (72, 7), "k_sdust_patch": (64, 8), "k_sdust_text": (64, 8)}      # (VGPRs at most, waves per SIMD at least); measured: 68, 19, 28


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "dust.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert all(k in rows for k in KERNELS), r.stdout[-2000:]
    return rows


@pytest.mark.parametrize("name", KERNELS)
def test_table_kernels_use_no_scratch_no_lds_and_no_agprs(resources, name):
    r = resources[name]
    print(name, r)
    assert r["scratch"] == 0 and r["lds"] == 0 and r["agpr"] == 0, r


@pytest.mark.parametrize("name", KERNELS)
def test_table_kernels_keep_their_registers(resources, name):
    r = resources[name]
    vgpr, occ = BOUNDS[name]
    assert r["vgpr"] <= vgpr and r["occ"] >= occ, r

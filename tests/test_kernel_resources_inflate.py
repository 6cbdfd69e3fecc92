"""Registers, spills and LDS of k_bgzf_inflate (kernels_inflate.hpp, hipcc's resource remarks, no GPU), after
tests/test_kernel_resources_bam.py.  The kernel keeps a member's 64-KiB history in LDS, one wave per workgroup: what DESIGN.md 8 (10)
states is two workgroups per CU -- at most 80 KiB of LDS each -- and registers that never limit that: no scratch, no AGPRs and at
most 128 VGPRs (the 4-waves-per-SIMD step; the LDS admits two waves per CU)."""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "reader.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m and m.group(1).strip() == "k_bgzf_inflate":
            return dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    raise AssertionError(r.stdout[-2000:])


def test_inflate_kernel_uses_no_scratch_and_no_agprs(resources):
    print(resources)
    assert resources["scratch"] == 0 and resources["agpr"] == 0, resources


def test_inflate_kernel_fits_two_workgroups_per_cu(resources):
    assert 65536 < resources["lds"] <= 80 * 1024 and resources["vgpr"] <= 128, resources

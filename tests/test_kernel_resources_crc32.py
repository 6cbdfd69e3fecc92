"""Registers, spills and LDS of k_crc32_ranges (kernels_crc32.hpp) and k_fx_names (kernels_fxscan.hpp), from hipcc's resource remarks
(no GPU), after tests/test_kernel_resources_inflate.py: no scratch, no AGPRs, at most 64 VGPRs each -- the eight-waves-per-SIMD step
the gather and scan kernels keep -- and at most 16 KiB of LDS for the CRC's tables."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_crc32_ranges", "k_fx_names")


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "reader.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    found = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m and m.group(1).strip() in KERNELS:
            found[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert set(found) == set(KERNELS), r.stdout[-2000:]
    return found


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_uses_no_scratch_and_no_agprs(resources, kernel):
    print(resources[kernel])
    assert resources[kernel]["scratch"] == 0 and resources[kernel]["agpr"] == 0, resources[kernel]


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_keeps_to_64_vgprs(resources, kernel):
    assert resources[kernel]["vgpr"] <= 64, resources[kernel]


def test_crc32_tables_fit_16_kib_of_lds(resources):
    assert 0 < resources["k_crc32_ranges"]["lds"] <= 16 * 1024, resources["k_crc32_ranges"]

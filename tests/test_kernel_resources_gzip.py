"""Registers, spills and LDS of the gzip kernels (kernels_gzip.hpp, hipcc's resource remarks, no GPU), after
tests/test_kernel_resources_inflate.py.  k_gz_inflate_spec keeps a ring of 32 Ki 16-bit symbols in LDS, one wave per workgroup: what
DESIGN.md 8 (11) states is two workgroups per CU -- more than 64 KiB and at most 80 KiB of LDS each -- and registers that never limit
that: no scratch, no AGPRs and at most 128 VGPRs.  k_gz_find holds only the tables (under 8 KiB); k_gz_window and k_gz_resolve use
no LDS; none of them spills."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_gz_find", "k_gz_inflate_spec", "k_gz_window", "k_gz_resolve")


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "reader.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m and m.group(1).strip() in KERNELS:
            out[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert sorted(out) == sorted(KERNELS), r.stdout[-2000:]
    return out


def test_gzip_kernels_use_no_scratch_and_no_agprs(resources):
    print(resources)
    for k in KERNELS:
        assert resources[k]["scratch"] == 0 and resources[k]["agpr"] == 0, (k, resources[k])


def test_gzip_decoder_fits_two_workgroups_per_cu(resources):
    r = resources["k_gz_inflate_spec"]
    assert 65536 < r["lds"] <= 80 * 1024 and r["vgpr"] <= 128, r
    assert resources["k_gz_find"]["lds"] <= 8 * 1024 and resources["k_gz_find"]["vgpr"] <= 128, resources["k_gz_find"]
    assert resources["k_gz_window"]["lds"] == 0 and resources["k_gz_resolve"]["lds"] == 0

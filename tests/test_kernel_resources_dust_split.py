"""Registers, spills and LDS of the kernels of the low-complexity scan in pieces (kernels_dust_split.hpp, hipcc's resource remarks, no GPU).
k_sdust_pieces keeps k_sdust's LDS layout (four lane-minor tables of 64 bytes per thread, 16 KiB per block of one wave), which is what
bounds the waves per CU; its registers must not grow past k_sdust's and nothing may spill.  The streaming kernels beside it (classify,
mask count, qualities, compact, scatter) stay without scratch, under the same register count and at the full eight waves per SIMD."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
K_SDUST_VGPRS = 49                                                  # k_sdust when the pieces were written
STREAMING = ("k_sdust_classify", "k_sdust_mask_count", "k_sdust_qual", "k_sdust_compact", "k_sdust_scatter")


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
    assert "k_sdust_pieces" in rows and "k_sdust" in rows, r.stdout[-2000:]
    return rows


def test_pieces_kernel_has_no_scratch_and_no_more_registers_than_k_sdust(resources):
    p, s = resources["k_sdust_pieces"], resources["k_sdust"]
    print("k_sdust_pieces:", p, "k_sdust:", s)
    assert p["scratch"] == 0 and p["agpr"] == 0, p
    assert p["vgpr"] <= K_SDUST_VGPRS and p["vgpr"] <= s["vgpr"], (p, s)
    assert p["lds"] == s["lds"] == 4 * 64 * 64                      # the same four tables


@pytest.mark.parametrize("name", STREAMING)
def test_streaming_kernels_use_no_scratch_no_lds_and_keep_full_occupancy(resources, name):
    r = resources[name]
    print(name, r)
    assert r["scratch"] == 0 and r["lds"] == 0 and r["agpr"] == 0, r
    assert r["vgpr"] <= K_SDUST_VGPRS and r["occ"] == 8, r          # (far inside the 8-wave step of 64)

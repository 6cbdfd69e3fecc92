"""Registers, spills and LDS of the adapter search's kernel (kernels_adapt.hpp, hipcc's resource remarks, no GPU): one wave per
read end, latency-bound on its lane-to-lane shuffle chain, so it needs every wave slot of a SIMD; the banded form (adapters over
64 bases) holds one window row of LQ_ADAPT_MAXLEN + 1 words in LDS."""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "adapt.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert "k_adapt<false>" in rows and "k_adapt<true>" in rows, r.stdout[-2000:]
    return rows


def test_adapter_kernel_keeps_full_occupancy_without_lds(resources):
    r = resources["k_adapt<false>"]
    assert r["vgpr"] <= 64 and r["scratch"] == 0 and r["occ"] == 8 and r["lds"] == 0, r


def test_banded_adapter_kernel_holds_one_row_in_lds(resources):
    r = resources["k_adapt<true>"]
    assert r["vgpr"] <= 64 and r["scratch"] == 0, r
    assert r["lds"] <= 4 * (4096 + 1) + 64, r                      # one row of the window, u32 per column

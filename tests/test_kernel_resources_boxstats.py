"""Registers, spills and LDS of the grouped box-plot kernels (kernels_boxstats.hpp) and of k_sdust_columns (kernels_dust_table.hpp), from
hipcc's resource remarks, no GPU.  None may spill, take AGPRs or use LDS.  The bounds are the VGPR step of the occupancy table that the
first clean build lands on, 8 waves per SIMD up to 64 VGPRs: k_box_stats 58 (six doubles of a box, the bisections' state, 64-bit places),
k_box_keys 18, k_box_flags 13, k_box_heads 10, k_sdust_columns 14.  The keys-only 64-bit instance of the engine's radix sort, which
boxstats.cpp is the first to use, must not spill either (136 VGPRs, three blocks per CU by its 47 KB of LDS like the pair sorts)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = {"boxstats.cpp": ["k_box_keys", "k_box_flags", "k_box_heads", "k_box_stats"], "dust.cpp": ["k_sdust_columns"]}
SORT = "k_is_pass<unsigned long, unsigned long, false>"
ALL = [(src, k) for src, ks in KERNELS.items() for k in ks]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    rows = {}
    for src in KERNELS:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:]
        for line in r.stdout.splitlines()[1:]:
            m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
            if m:
                rows[(src, m.group(1).strip())] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert set(ALL) | {("boxstats.cpp", SORT)} <= set(rows), sorted(rows)
    return rows


@pytest.mark.parametrize("src,kernel", ALL)
def test_box_kernels_use_no_scratch_no_agprs_and_no_lds(resources, src, kernel):
    r = resources[(src, kernel)]
    assert r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, r


@pytest.mark.parametrize("src,kernel", ALL)
def test_box_kernels_keep_full_occupancy(resources, src, kernel):
    r = resources[(src, kernel)]
    assert r["vgpr"] <= 64 and r["occ"] == 8, r


def test_the_keys_only_sort_of_64_bit_keys_does_not_spill(resources):
    r = resources[("boxstats.cpp", SORT)]
    assert r["scratch"] == 0 and r["agpr"] == 0 and r["occ"] >= 3, r

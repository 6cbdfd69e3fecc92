"""Registers, spills and LDS of the table reader's kernels (kernels_csv.hpp) and of the f64 box kernels (kernels_boxstats_f64.hpp), from
hipcc's resource remarks at gfx950, no GPU, after tests/test_kernel_resources_polread.py.  The budgets are the first clean build's
(DESIGN.md 8 (21)): no scratch and no AGPRs anywhere; LDS only in k_csv_pack, the block scan's word per wave; every kernel within 4 VGPRs
of what that build gave it and at 8 waves per SIMD.  The thousandths kernels that boxstats_f64.cpp compiles a second time, in a
namespace of their own, keep the registers tests/test_kernel_resources_boxstats.py states for boxstats.cpp's."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# VGPRs of the build these budgets were read from (hipcc's remarks for the code as written), each allowed a margin of 4
VGPRS = {"csv.cpp": {"k_csv_marks": 17, "k_csv_rows": 12, "k_csv_starts": 16, "k_csv_parse": 28, "k_csv_lengths": 20, "k_csv_pack": 44},
         "boxstats_f64.cpp": {"k_boxd_keys": 18, "k_boxd_rekey": 8, "k_boxd_flags": 12, "k_boxd_stats": 46, "lq_box_thou::k_box_heads": 10}}
MARGIN = 4
ALL = [(src, k) for src, ks in VGPRS.items() for k in ks]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    rows = {}
    for src in VGPRS:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:]
        for line in r.stdout.splitlines()[1:]:
            m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
            if m:
                rows[(src, m.group(1).strip())] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert set(ALL) <= set(rows), sorted(rows)
    return rows


@pytest.mark.parametrize("src,kernel", ALL)
def test_csv_kernels_use_no_scratch_and_no_agprs(resources, src, kernel):
    r = resources[(src, kernel)]
    print(kernel, r)
    assert r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == (32 if kernel == "k_csv_pack" else 0), r


@pytest.mark.parametrize("src,kernel", ALL)
def test_registers_stay_within_a_small_margin_of_the_first_build(resources, src, kernel):
    r = resources[(src, kernel)]
    assert r["vgpr"] <= VGPRS[src][kernel] + MARGIN and r["occ"] == 8, (r, VGPRS[src][kernel])


def test_the_kernels_csv_cpp_borrows_are_polread_cpp_s(resources):
    """k_pol_unkey and k_pol_nxx are compiled into csv.cpp from kernels_polread.hpp as they are: the registers
    tests/test_kernel_resources_polread.py states"""
    assert resources[("csv.cpp", "k_pol_unkey")]["vgpr"] <= 7 + MARGIN and resources[("csv.cpp", "k_pol_nxx")]["vgpr"] <= 14 + MARGIN
    assert resources[("csv.cpp", "k_pol_nxx")]["scratch"] == 0

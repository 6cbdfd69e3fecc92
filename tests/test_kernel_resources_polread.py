"""Registers, spills and LDS of the Sequel platform QC's kernels (kernels_polread.hpp, hipcc's resource remarks, no GPU), after
tests/test_kernel_resources_fxscan.py.  The budgets are the first clean build's: no scratch and no AGPRs anywhere; LDS
only the block scan's word per wave; every kernel within 4 VGPRs of what that build gave it; the streaming kernels at 8 waves;
k_pol_fields -- a byte walk with a handful of live positions -- at 7 waves or more, where its scalar registers put it."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# VGPRs of the build these budgets were read from (hipcc's remarks for the code as written), each allowed a margin of 4
VGPRS = {"k_pol_fields": 44, "k_pol_compact": 34, "k_pol_keys": 15, "k_pol_rekey": 8, "k_pol_order": 14, "k_pol_heads": 10, "k_pol_walk": 30,
         "k_pol_ispol": 8, "k_pol_pack": 42, "k_pol_unkey": 7, "k_pol_nxx": 14}
MARGIN = 4
KERNELS = tuple(VGPRS)
STREAMING = KERNELS[1:]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "polread.cpp"], stdout=subprocess.PIPE,
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


def test_polread_kernels_use_no_scratch_and_no_agprs(resources):
    for k in KERNELS:
        print(k, resources[k])
        assert resources[k]["scratch"] == 0 and resources[k]["agpr"] == 0 and resources[k]["lds"] <= 32, (k, resources[k])


def test_registers_stay_within_a_small_margin_of_the_first_build(resources):
    for k, v in VGPRS.items():
        assert resources[k]["vgpr"] <= v + MARGIN, (k, resources[k], v)


def test_occupancy_is_the_first_build_s(resources):
    for k in STREAMING:
        assert resources[k]["occ"] == 8, (k, resources[k])
    assert resources["k_pol_fields"]["occ"] >= 7, resources["k_pol_fields"]      # (7: its scalar registers, not its 44 VGPRs)

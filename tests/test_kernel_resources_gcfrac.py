"""Registers, spills and LDS of the GC fraction step's kernels (kernels_gc.hpp, hipcc's resource remarks, no GPU).  All three
are streaming kernels without LDS: what hides their load latency is waves per SIMD, so the bounds below are the VGPR steps of
the occupancy table (8 waves up to 64 VGPRs, 7 up to 72), read off the first clean build: k_gc_reads 68 VGPRs (four 16-byte
loads in flight per lane plus the masks of a read's head and tail), k_gc_windows 39, k_gc_draw 16."""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "gc.cpp"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), agpr=int(m.group(3)), scratch=int(m.group(4)), occ=int(m.group(5)), lds=int(m.group(6)))
    assert {"k_gc_reads", "k_gc_windows", "k_gc_draw"} <= set(rows), r.stdout[-2000:]
    return rows


@pytest.mark.parametrize("kernel", ["k_gc_reads", "k_gc_windows", "k_gc_draw"])
def test_gc_kernels_use_no_scratch_and_no_lds(resources, kernel):
    r = resources[kernel]
    assert r["scratch"] == 0 and r["lds"] == 0 and r["agpr"] == 0, r


def test_read_count_kernel_keeps_seven_waves_per_simd(resources):
    r = resources["k_gc_reads"]
    assert r["vgpr"] <= 72 and r["occ"] >= 7, r                     # 16 VGPRs of loaded bases per lane; 72 is the 7-wave step


def test_window_and_draw_kernels_keep_full_occupancy(resources):
    for name in ("k_gc_windows", "k_gc_draw"):
        r = resources[name]
        assert r["vgpr"] <= 64 and r["occ"] == 8, (name, r)

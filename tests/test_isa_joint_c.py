"""CPU: the joint phase-C sweep of k_solve_lds<2, 512, false, 1> in tools/isa_check.py's report.

The kernel forms the excitation of both bins of a thread in one node sweep.  Its ring has kRingC
slots of one (node, bin), two rows each, consumed and refilled one at a time, so every wait inside
the loop leaves the other kRingC - 1 slots' loads outstanding: (6 - 1) x 2 = 10 (`ringCJ=`).  The
sweep holds both bins' sums and F (80 VGPRs more than one bin's) and must not push anything to
scratch: the kernel takes 255 VGPRs with no spill, and bin 1's excitation crosses bin 0's solve in
global memory, not in registers."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

JOINT = "k_solve_lds<2, 512, false, 1>"
SPLIT = "k_solve_lds_split<2, 512, false, 1>"


@pytest.fixture(scope="module")
def report():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py")], capture_output=True, text=True,
                       timeout=600)
    return p.returncode, p.stdout + p.stderr[-2000:]


def line_of(out, kernel):
    return next(ln for ln in out.splitlines() if kernel in ln)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_joint_loop_keeps_its_ring_full(report):
    rc, out = report
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    _, ring_c = isa_check.ring_depths()
    slots, per_slot = ring_c, 2   # one (node, bin) per slot, its two transverse rows
    need = (slots - 1) * per_slot
    assert need == 10, need
    line = line_of(out, JOINT)
    print(line)
    m = re.search(r"ringCJ=(\d+)>=(\d+)", line)
    assert m, line
    assert int(m.group(2)) == need and int(m.group(1)) >= need, line
    assert rc == 0 and "FAIL" not in out, out[-3000:]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_joint_kernel_has_no_scratch_and_no_spill(report):
    rc, out = report
    line = line_of(out, JOINT)
    assert "in_flight=  0 in_loops=  0" in line, line
    assert re.search(r"scratch=\s*0\b", line), line
    assert "vgpr=255 spill=0" in line, line   # DESIGN.md §5, "One phase-C node sweep for both bins"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_split_kernel_is_still_built_and_clean(report):
    """The one-sweep-per-bin form (rh_set_solver(ctx, 8)) stays compiled, spill-free as before."""
    rc, out = report
    line = line_of(out, SPLIT)
    assert "in_flight=  0 in_loops=  0" in line, line
    assert "vgpr=256 spill=0" in line, line

"""CPU: the depth the wave-table prefetch rings of the benched fixed points really keep
(tools/isa_check.py, `rings=` / `ringA=` / `ringC=`).

A ring D slots deep hides latency only if the wait before slot r's rows leaves the loads of the
other D - 1 slots outstanding.  hipcc counts `s_waitcnt vmcnt(N)` exactly along straight code, but
at a merge point whose arms issued different numbers of loads (a tail guard per slot, a load under
a branch) it takes the smallest count, and the ring is then drained once a round or once a node
(DESIGN.md §5).  The gate: in k_solve_lds<2, 512, false, 1> (C2) and k_solve_lds<2, 128, true, 1>
(C4) the smallest vmcnt(N) waited for inside the phase-A transverse ring and inside the phase-C
node loop, with loads of the loop in flight, is at least (ring depth - 1) x loads per slot:
12 = 3 x (2 rows x 2 bins) with kRingA1 = 4, and 10 = 5 x 2 rows with kRingC = 6."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

BENCHED = ("k_solve_lds<2, 512, false, 1>", "k_solve_lds<2, 128, true, 1>")


@pytest.fixture(scope="module")
def report():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py")], capture_output=True, text=True,
                       timeout=600)
    return p.returncode, p.stdout + p.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_ring_depth_gate(report):
    rc, out = report
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    ring_a, ring_c = isa_check.ring_depths()
    need = {"A": (ring_a - 1) * 4, "C": (ring_c - 1) * 2}
    assert need == {"A": 12, "C": 10}, need   # today's depths: a change of kRingA1 / kRingC moves the bound with it
    for k in BENCHED:
        line = next(ln for ln in out.splitlines() if k in ln)
        print(line)
        for ph in "AC":
            m = re.search(r"ring%s=(\d+)>=(\d+)" % ph, line)
            assert m, (ph, line)   # "?": the loop was not found or never waits with a load in flight
            assert int(m.group(2)) == need[ph], line
            assert int(m.group(1)) >= need[ph], line
    assert rc == 0 and "FAIL" not in out, out[-3000:]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_benched_kernels_have_no_scratch_in_loops(report):
    rc, out = report
    for k in BENCHED:
        line = next(ln for ln in out.splitlines() if k in ln)
        assert "in_flight=  0 in_loops=  0" in line, line


def test_ring_depth_measure_on_a_known_loop():
    """The measure itself on hand-written loops: a ring that stays full, one drained at its head."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    load = "\tbuffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen"
    full = [".LBB0_1:", "\ts_waitcnt vmcnt(2)", load, load, "\ts_waitcnt vmcnt(2)", load, load, "\ts_cbranch_scc1 .LBB0_1"]
    assert isa_check.ring_depth(full, 0, len(full) - 1) == (4, 2)
    drained = [".LBB0_1:", "\ts_waitcnt vmcnt(0)", load, load, "\ts_waitcnt vmcnt(2)", load, load, "\ts_cbranch_scc1 .LBB0_1"]
    assert isa_check.ring_depth(drained, 0, len(drained) - 1) == (4, 0)
    idle = [".LBB0_1:", load, "\ts_waitcnt vmcnt(0)", "\ts_waitcnt vmcnt(0)", "\ts_cbranch_scc1 .LBB0_1"]
    assert isa_check.ring_depth(idle, 0, len(idle) - 1) == (1, 0)

"""CPU: phase B of k_solve_lds<2, 512, false, 1> in tools/isa_check.py's report.

Phase B runs on one wave (lanes 0..nn-1, then lanes 0..35) while the other seven wait at its barriers,
and nothing else fits on the CU beside the kernel, so every dependent LDS round trip in it is step
time.  `phaseB_lgkm_waits=` counts the `s_waitcnt lgkmcnt` between the barrier that closes phase A and
the one that closes phase B.  The gate is 40: well under half the 101 of the kernel before its reads
were batched (94 in the per-node stage, 7 in the node sum).

With the wave partials read ahead of their adds, the node's Bmat in registers for the 36 translate
entries and the node sum in batches of 16 the count is 34: 16 in the per-node stage, 18 in
the node sum, whose batches are waited for read by read as they return (4 round trips instead of 31).

The kernel's other fields on that line stay what they were: rings full, no scratch, 255 VGPRs, no
spill."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

JOINT = "k_solve_lds<2, 512, false, 1>"
MAX_WAITS = 40


@pytest.fixture(scope="module")
def report():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py")], capture_output=True, text=True,
                       timeout=600)
    return p.returncode, p.stdout + p.stderr[-2000:]


def line_of(out, kernel):
    return next(ln for ln in out.splitlines() if kernel in ln)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_phase_b_waits_are_batched(report):
    rc, out = report
    line = line_of(out, JOINT)
    print(line)
    m = re.search(r"phaseB_lgkm_waits=(\d+)", line)
    assert m, line
    assert int(m.group(1)) <= MAX_WAITS, line


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_ring_and_spill_fields_unchanged(report):
    rc, out = report
    line = line_of(out, JOINT)
    assert "in_flight=  0 in_loops=  0" in line, line
    assert re.search(r"scratch=\s*0\b", line), line
    assert "ringA=12>=12 ringC=10>=10 ringCJ=10>=10 vgpr=255 spill=0" in line, line
    assert rc == 0 and "FAIL" not in out, out[-3000:]


def test_the_count_finds_phase_b():
    """The counter on a body it can be checked on by hand: phase B is the stretch from the barrier
    before the only run of field loads to the second barrier after it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    loads = ["\tglobal_load_dwordx2 v[4:5], v[2:3], off"] * 16
    body = (["\ts_waitcnt lgkmcnt(0)", "\ts_barrier", "\ts_waitcnt lgkmcnt(0)", "\ts_barrier"] + loads
            + ["\ts_waitcnt vmcnt(0)", "\ts_waitcnt lgkmcnt(2)", "\ts_barrier", "\ts_waitcnt vmcnt(0) lgkmcnt(0)", "\ts_barrier",
               "\ts_waitcnt lgkmcnt(0)", "\ts_barrier"])
    assert isa_check.phase_b_lgkm_waits(body) == 2
    assert isa_check.phase_b_lgkm_waits(body[:4]) is None

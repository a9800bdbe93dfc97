"""CPU: the LU's complex updates in the device code of k_solve_lds<2, 512, false, 1> are fused.

rh::lu_solve<6> (csrc/rh_device.h) writes each update a - l u as four FMAs (msub).  Written as
sub(a, mul(l, u)) the compiler made v_mul_f64, v_fma_f64, v_add_f64 of each component: two multiplies and
two adds more per update, 170 of each over the 85 updates of a 6 x 6 solve (55 in the elimination, 15 on the
right-hand side, 15 in the back substitution).  profiles/r13_v1/isa_counts_parent.txt holds the kernel's static
counts before the change, measured with the same counter (tools/isa_check.py, fp64_counts); the kernel must
now show at least 150 fewer of each -- the 170 expected, with room for scheduling differences.

Needs hipcc; compiles rh_solve_fast.hip alone, with the flags the build gives it.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

JOINT = "k_solve_lds<2, 512, false, 1>"
LESS = 150


def parent_counts():
    with open(os.path.join(ROOT, "profiles", "r13_v1", "isa_counts_parent.txt")) as fh:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^v_(\w+)_f64 (\d+)$", fh.read(), re.M)}


@pytest.fixture(scope="module")
def counts():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check as I
    flags = dict(I.G.UNITS)["rh_solve_fast.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "fast.s")
        subprocess.run([I.G.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "--offload-device-only", "-S",
                        "-o", asm, os.path.join(I.G.CSRC, "rh_solve_fast.hip")], check=True, timeout=600)
        with open(asm) as fh:
            ks = I.kernels(fh.read().split("\n"))
    body = [b for n, b in ks.items() if JOINT in I.demangle(n)]
    assert len(body) == 1, sorted(I.demangle(n) for n in ks)
    return dict(zip(("mul", "add", "fma"), I.fp64_counts(body[0])))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_lu_updates_are_fused(counts):
    parent = parent_counts()
    assert set(parent) == {"mul", "add", "fma"}, parent
    print("parent", parent, "now", counts)
    assert counts["mul"] <= parent["mul"] - LESS, (counts, parent)
    assert counts["add"] <= parent["add"] - LESS, (counts, parent)


def test_the_counter_counts_whole_mnemonics():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check as I
    body = ["\tv_mul_f64 v[0:1], v[2:3], v[4:5]", "\tv_fma_f64 v[0:1], v[2:3], v[4:5], v[0:1]", "\tv_add_f64 v[0:1], v[2:3], v[4:5]",
            "\tv_add_f64 v[0:1], v[2:3], -v[4:5]", "\tv_mul_f32 v0, v1, v2", "\tv_pk_mul_f32 v[0:1], v[2:3], v[4:5]",
            "\t; v_mul_f64 in a comment", "\tv_fmac_f64_e32 v[0:1], v[2:3], v[4:5]", "\tv_div_fmas_f64 v[0:1], v[2:3], v[4:5], v[6:7]"]
    assert I.fp64_counts(body) == (1, 2, 2)   # (mul, add, fma with fmac)

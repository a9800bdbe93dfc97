"""CPU: the row exchange of rh::lu_solve<6> (csrc/rh_device.h) entered for rows no lane pivots to.

On the device the exchange of step k with candidate row i is entered by a whole wave whenever one of its
lanes pivots to row i; every other lane runs the block's selects with `sw` false.  The form is safe only
if such a lane's bits are then what they would have been without the block.  tools/lu_rows_host.cpp
compiles the header for the host twice: with the host's one-lane wave_any (a block is entered only by a
lane that exchanges), and with -DRH_HOST_WAVE_ANY_TRUE (every block of every step is entered, as for a
lane whose wave mates pivot to every row).  On every system of tests/helpers/lu_cases.py -- families P,
T, S, C and Z, every row order of every_step_perms(), the layouts of tests/test_gpu_lu.py with singular
bins -- x and ok of the two builds are equal bit for bit, for the per-row form and for the chain form
kept beside it (k_solve_cases<2>, <8>), and the two forms are equal to each other.  Every system also
passes the criterion of tests/test_lu_fma_host.py: backward error at most 8 max(worst eta of
numpy.linalg.solve on that family, u), no NaN and no zero-pivot verdict on a regular system, the verdict
on every exactly singular one.  No tolerance of its own.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lu_cases as L   # noqa: E402

U = L.U
FORMS = ["rh_lu_rows6_host", "rh_lu_chain6_host"]


def _build(defines):
    out = os.path.join(tempfile.mkdtemp(), "lu_rows_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", *defines, "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "lu_rows_host.cpp")], check=True)
    lib = ctypes.CDLL(out)
    for name in FORMS:
        f = getattr(lib, name)
        f.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
        f.restype = None
    lib.rh_lu_rows_enters_all.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def libs():
    """(the build whose blocks are entered only by a lane that exchanges, the build that enters every block)"""
    own, every = _build([]), _build(["-DRH_HOST_WAVE_ANY_TRUE"])
    assert own.rh_lu_rows_enters_all() == 0 and every.rh_lu_rows_enters_all() == 1
    return own, every


def solve(lib, entry, A, b):
    A = np.ascontiguousarray(A, dtype=complex)
    b = np.ascontiguousarray(b, dtype=complex)
    x = np.zeros_like(b)
    ok = np.zeros(len(A), dtype=np.int32)
    getattr(lib, entry)(len(A), A.ctypes.data, b.ctypes.data, x.ctypes.data, ok.ctypes.data)
    return x, ok.astype(bool)


@pytest.fixture(scope="module")
def systems():
    """Every system of the helper, once, each set with numpy's eta; the worst per family over all sets."""
    rng = np.random.default_rng(4)
    fam, name, A = [], [], []
    for f, make in L.REGULAR6.items():
        d = make(12)
        fam += [f] * len(d)
        name += list(d)
        A += [d[k] for k in d]
    out = [L.Systems(np.array(A), L._cplx(rng, len(A), 6), fam, name)]
    # every row order of a dominant matrix that exchanges at every step 0..4
    B = L._dominant(np.random.default_rng(6))
    ev = L.every_step_perms()
    out.append(L.Systems(np.array([B[list(p)] for p in ev]), L._cplx(rng, len(ev), 6), ["P"] * len(ev),
                         ["every " + "".join(map(str, p)) for p in ev]))
    # family Z alone, then among the layouts' regular bins
    Z = L.family_Z(3)
    out.append(L.Systems(np.array([Z[k] for k in Z]), np.ones([len(Z), 6], dtype=complex), ["Z"] * len(Z), list(Z),
                         np.ones(len(Z), dtype=bool)))
    nw = 200
    out += [L.layout(nw, 0), L.layout(nw, 2), L.with_singular(L.layout(nw, 1), [5, 70, nw - 1])]
    worst = {}
    for s in out:
        s.eta_np, w = L.numpy_eta(s) if not s.singular.all() else (None, {})
        for f, v in w.items():
            worst[f] = max(worst.get(f, 0.0), v)
    assert set(worst) == set(L.REGULAR6) and sum(int(s.singular.sum()) for s in out) == 6
    assert len(ev) > 0 and all(len(L.device_lu6(a, np.ones(6))[1]) == 5 for a in out[1].A)
    return out, worst


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_entering_every_block_changes_no_bit(libs, systems):
    own, every = libs
    ss, _ = systems
    for ic, s in enumerate(ss):
        ref = solve(own, FORMS[0], s.A, s.b)
        for lib, tag in ((own, "own"), (every, "every")):
            for entry in FORMS:
                x, ok = solve(lib, entry, s.A, s.b)
                assert np.array_equal(ok, ref[1]), (ic, tag, entry, np.nonzero(ok != ref[1])[0])
                if not same_bits(x, ref[0]):
                    bad = np.nonzero((x.view(np.uint64) != ref[0].view(np.uint64)).any(axis=1))[0]
                    raise AssertionError((ic, tag, entry, [(int(b), s.name[b]) for b in bad[:8]]))


@pytest.mark.parametrize("entry", FORMS)
def test_every_system_meets_the_gepp_criterion(libs, systems, entry):
    """The criterion of tests/test_lu_fma_host.py, on the build that enters every block."""
    _, every = libs
    ss, worst = systems
    bound = L.gepp_bound(worst)
    for ic, s in enumerate(ss):
        x, ok = solve(every, entry, s.A, s.b)
        assert np.array_equal(ok, ~s.singular), (entry, ic, np.nonzero(ok == s.singular)[0])
        reg = np.nonzero(~s.singular)[0]
        assert np.all(np.isfinite(x[reg])), (entry, ic)
        if not len(reg):
            continue
        eta = np.full(s.nw, np.nan)
        for b in reg:
            eta[b] = L.backward_error(s.A[b], s.b[b], x[b])
        print(L.table_row(f"{entry} set {ic}", s, eta, {f: worst[f] for f in set(s.fam[reg])}))
        for b in reg:
            assert eta[b] <= bound[s.fam[b]], (entry, ic, b, s.fam[b], s.name[b], eta[b], bound[s.fam[b]])
        for b in [b for b in reg if s.fam[b] == "C"][:16]:
            kinf = np.linalg.cond(s.A[b], np.inf)
            assert L.forward_error(s.A[b], s.b[b], x[b]) <= 64 * kinf * U, (entry, ic, b)

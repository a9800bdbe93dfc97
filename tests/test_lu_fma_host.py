"""CPU: the header's own rh::lu_solve<6> and rh::lu_factor<6> / rh::lu_apply<6> (csrc/rh_device.h, compiled for
the host with g++ through tools/lu_host.cpp) on every system of tests/helpers/lu_cases.py.

The LU's updates a - l u are four FMAs each, in an order the source fixes.  That changes last bits, so the
statements the kernels run are held here, without a GPU, to the criterion tests/test_gpu_lu.py holds the
device to: the backward error (residual in mpmath) of every regular system is at most
8 max(worst eta of numpy.linalg.solve on that family, u), no regular system gives a NaN or a zero-pivot
verdict, and every exactly singular one gives the verdict (lu_solve's `false`, NaN in every row from
lu_factor / lu_apply).  No tolerance of its own.
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
ENTRIES = ["rh_lu_solve6_host", "rh_lu_factor_apply6_host"]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(), "lu_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "lu_host.cpp")], check=True)
    lib = ctypes.CDLL(out)
    for name in ENTRIES:
        f = getattr(lib, name)
        f.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
        f.restype = None
    return lib


def solve(lib, entry, A, b):
    """(x [n][6], ok [n]) of the host build on the stack A [n][6][6], b [n][6]."""
    A = np.ascontiguousarray(A, dtype=complex)
    b = np.ascontiguousarray(b, dtype=complex)
    x = np.zeros_like(b)
    ok = np.zeros(len(A), dtype=np.int32)
    getattr(lib, entry)(len(A), A.ctypes.data, b.ctypes.data, x.ctypes.data, ok.ctypes.data)
    return x, ok.astype(bool)


@pytest.fixture(scope="module")
def systems():
    """Every system of the helper, once: the regular families as tests/test_lu_cases.py draws them, and the
    three cases of tests/test_gpu_lu.py on a grid of three full waves and a ragged one (the quiet, busy and
    mixed waves, the pool, and family Z in three bins), each with numpy's eta; the worst per family over all."""
    rng = np.random.default_rng(4)
    fam, name, A = [], [], []
    for f, make in L.REGULAR6.items():
        d = make(12)
        fam += [f] * len(d)
        name += list(d)
        A += [d[k] for k in d]
    A = np.array(A)
    out = [L.Systems(A, L._cplx(rng, len(A), 6), fam, name)]
    nw = 200
    out += [L.layout(nw, 0), L.layout(nw, 2), L.with_singular(L.layout(nw, 1), [5, 70, nw - 1])]
    worst = {}
    for s in out:
        s.eta_np, w = L.numpy_eta(s)
        for f, v in w.items():
            worst[f] = max(worst.get(f, 0.0), v)
    assert set(worst) == set(L.REGULAR6) and out[-1].singular.sum() == 3
    return out, worst


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_system_meets_the_gepp_criterion(lib, systems, entry):
    ss, worst = systems
    bound = L.gepp_bound(worst)
    for ic, s in enumerate(ss):
        x, ok = solve(lib, entry, s.A, s.b)
        assert np.array_equal(ok, ~s.singular), (entry, ic, np.nonzero(ok == s.singular)[0])
        reg = np.nonzero(~s.singular)[0]
        assert np.all(np.isfinite(x[reg])), (entry, ic)
        if entry == "rh_lu_factor_apply6_host":      # no flag is carried: the NaN is in the numbers
            assert np.all(np.isnan(x[s.singular].real)) and np.all(np.isnan(x[s.singular].imag)), (entry, ic)
        eta = np.full(s.nw, np.nan)
        for b in reg:
            eta[b] = L.backward_error(s.A[b], s.b[b], x[b])
        print(L.table_row(f"{entry} set {ic}", s, eta, {f: worst[f] for f in set(s.fam[reg])}))
        for b in reg:
            assert eta[b] <= bound[s.fam[b]], (entry, ic, b, s.fam[b], s.name[b], eta[b], bound[s.fam[b]])
        for b in [b for b in reg if s.fam[b] == "C"][:16]:
            kinf = np.linalg.cond(s.A[b], np.inf)
            assert L.forward_error(s.A[b], s.b[b], x[b]) <= 64 * kinf * U, (entry, ic, b)


def test_singular_family_alone(lib):
    """Family Z by name: the zero matrix, a zero column, the exact rank-5 matrix."""
    Z = L.family_Z(3)
    A = np.array([Z[k] for k in Z])
    b = np.ones([len(A), 6], dtype=complex)
    _, ok = solve(lib, ENTRIES[0], A, b)
    assert not ok.any(), dict(zip(Z, ok))
    x, ok = solve(lib, ENTRIES[1], A, b)
    assert not ok.any() and np.all(np.isnan(x.real)) and np.all(np.isnan(x.imag)), dict(zip(Z, ok))


"""CPU check of the general mooring system and the N-FOWT mean-offset Newton of the device
(raft-teststuff_amd/csrc/rh_moor_array.h) against the Python they restate (raft/mooring.py,
raft/dsolve.py, Model.solveStatics): the header is compiled for the host with g++
(tools/moor_array_host.cpp), so the same line solve, free-point equilibrium, condensation and
Newton the GPU runs are compared here without a GPU.  Also the flattener's tables, the refusals
and limits of raft/mooring_array_device.py, and the new ABI symbols."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import moor_array_cases as C   # noqa: E402

_p, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(), "moor_array_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "moor_array_host.cpp")], check=True)
    L = ctypes.CDLL(out)
    L.rh_moor_aline_host.argtypes = [_p, _p] + [_d] * 7 + [_p]
    L.rh_moor_aline_host.restype = None
    L.rh_moor_array_eval_host.argtypes = [_p] * 4 + [_i] + [_p] * 9
    L.rh_moor_array_eval_host.restype = None
    L.rh_array_statics_solve_host.argtypes = [_p] * 14
    L.rh_array_statics_solve_host.restype = None
    L.rh_moor_array_lu_host.argtypes = [_p, _i, _i, _i]
    L.rh_moor_array_lu_host.restype = _i
    return L


def P(a):
    return None if a is None else a.ctypes.data


def rec_args(rec):
    ri = np.array([rec.nbody, rec.npoint, rec.nline, rec.nfree, rec.free_sys], dtype=np.int32)
    rd = np.array([rec.g, rec.rho, rec.free_tol, rec.free_depth], dtype=float)
    return ri, rd


def eval_host(L, rec, r6, warm, free, jac=True):
    ri, rd = rec_args(rec)
    nD, nl = 6 * rec.nbody, rec.nline
    r6 = np.ascontiguousarray(r6, dtype=float).reshape(1, nD)
    warm, free = np.array(warm, dtype=float).reshape(nl, 2).copy(), np.array(free, dtype=float).reshape(-1, 3).copy()
    F, K, T, J = np.zeros(nD), np.zeros([nD, nD]), np.zeros(2 * nl), np.zeros([2 * nl, nD])
    nev, st = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    L.rh_moor_array_eval_host(P(ri), P(rd), P(rec.point), P(rec.line), 1, P(r6), P(warm), P(free), P(F), P(K), P(T),
                              P(J) if jac else None, P(nev), P(st))
    return dict(F=F, K=K, T=T, J=J, nev=int(nev[0]), status=int(st[0]), warm=warm, free=free)


# ------------------------------------------------------------------------------ line solve
def line_pairs():
    """80 seeded (A, B, L, depth) end pairs: both orderings of the ends, seabed contact (the lower end
    on the seabed, L between the chord and the folded length LH + dz) and suspended (both ends off
    the seabed, as a free-free line has them).  Seed 79 replaces seed 31: with 31 (and most seeds,
    about 5 draws in 80) raft.mooring.catenary itself runs out of iterations on a long, flat seabed
    line; with 79 the Python solves every draw, and every draw is compared."""
    rng = np.random.default_rng(79)
    rows = []
    for kind in ["seabed", "suspended"]:
        for k in range(40):
            depth = rng.uniform(100.0, 600.0)
            lo = np.array([rng.uniform(-500, 500), rng.uniform(-500, 500), -depth if kind == "seabed" else
                           -depth * rng.uniform(0.2, 0.9)])
            up = lo + np.array([rng.uniform(50, 900) * rng.choice([-1, 1]), rng.uniform(0, 400), 0.0])
            up[2] = rng.uniform(lo[2] + 5.0, -5.0)
            LH, chord = np.hypot(up[0] - lo[0], up[1] - lo[1]), np.linalg.norm(up - lo)
            Ln = chord * rng.uniform(1.01, 1.25)
            if kind == "seabed":
                Ln = chord + rng.uniform(0.1, 0.7) * (LH + up[2] - lo[2] - chord)
            rows.append((kind, up, lo, Ln, depth) if k % 2 else (kind, lo, up, Ln, depth))
    return rows


def test_general_line_solve_matches_python(lib, monkeypatch):
    """fA, fB, Ku, TA, TB and the warm state to 1e-12 relative with equal catenary iteration counts."""
    import raft.mooring as M
    count = [0]
    real = M._catenary_residual

    def counted(*a):
        count[0] += 1
        return real(*a)
    monkeypatch.setattr(M, "_catenary_residual", counted)
    kinds, swaps, worst = set(), set(), 0.0
    for kind, A, B, Ln, depth in line_pairs():
        ms = M.MooringSystem(depth=depth)
        ms.add_line_type("chain", 0.15, 300.0, 5.0e8)
        ln = ms.add_line(Ln, "chain", ms.add_point(M.Point.FREE, A), ms.add_point(M.Point.FREE, B))
        count[0] = 0
        ln.static_solve(depth, 1e-5)
        out = np.zeros(21)
        A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
        lib.rh_moor_aline_host(P(A), P(B), Ln, 5.0e8, ms.line_types["chain"]["w"], depth, 1e-5, 0.0, 0.0, P(out))
        assert out[20] == 0 and out[19] == count[0], (kind, out[19], count[0])
        ref = np.concatenate([ln.fA, ln.fB, ln.KA.ravel(), [ln.TA, ln.TB, ln.HF, ln.VF]])
        np.testing.assert_allclose(out[:19], ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        np.testing.assert_array_equal(ln.KAB, -ln.KA)
        worst = max(worst, C.rel(out[:19], ref))
        kinds.add((kind, bool(ln.fA[2] != 0.0 or kind == "suspended")))
        swaps.add(bool(B[2] < A[2]))
    assert swaps == {True, False} and {k for k, _ in kinds} == {"seabed", "suspended"}
    print(f"general line solve: worst residual {worst:.2e}")


# ------------------------------------------------------------------------------ systems
def check_system(L, ms, X_ref, n, seed, label):
    """n seeded poses, each started from the system's state at its reference poses."""
    from raft.mooring_array_device import array_state, flatten_array
    rec = flatten_array(ms)
    state = C.get_state(ms)
    warm0, free0 = array_state(rec)
    worst = np.zeros(5)
    for r6 in C.seeded_poses(X_ref, n, seed):
        ref = C.python_eval(ms, r6, state)
        got = eval_host(L, rec, r6, warm0, free0)
        assert got["status"] == 0 and got["nev"] == ref["nev"], (label, got["status"], got["nev"], ref["nev"])
        errs = [C.rel(got["F"], ref["F"]), C.rel(got["K"], ref["K"]), C.rel(got["T"], ref["T"]),
                C.rel(got["free"], ref["free"]), C.rel(got["J"], ref["J"])]
        worst = np.maximum(worst, errs)
        assert max(errs[:4]) < C.TOL and errs[4] < C.TOL_J, (label, errs)
        np.testing.assert_allclose(got["warm"], ref["warm"], rtol=1e-9)
    C.set_state(ms, state)
    print(f"{label}: worst F, K, T, free, J residuals {worst}")
    return rec


def test_farm_array_system_matches_python(lib):
    """VolturnUS-S_farm's array system (2 bodies, 2 clump free points, 7 lines) at 10 seeded pose pairs."""
    m = C.farm_model()
    rec = check_system(lib, m.ms, np.array([[0.0, 0, 0, 0, 0, 0], [1600.0, 0, 0, 0, 0, 0]]), 10, 5, "farm")
    assert (rec.nbody, rec.nfree, rec.nline) == (2, 2, 7)


@pytest.mark.parametrize("name", ["clump", "two_bodies", "same_body", "chain8"])
def test_synthetic_systems_match_python(lib, name):
    ms, X_ref = C.synthetic_systems()[name]
    rec = check_system(lib, ms, X_ref, 6, 17, name)
    assert rec.nfree == {"clump": 1, "two_bodies": 0, "same_body": 0, "chain8": 8}[name]


# ------------------------------------------------------------------------------ mean offsets
def statics_host(L, m, case):
    rec, subs, X_ref, K_hs, F_const, warm0, free0 = m._statics_array_inputs([dict(case)])
    ri, rd = rec_args(rec)
    nD = 6 * rec.nbody
    X, warm, free = np.zeros(nD), np.zeros([rec.nline, 2]), np.zeros([max(rec.nfree, 1), 3])
    it, st = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    args = [np.ascontiguousarray(a, dtype=float) for a in (X_ref, K_hs, F_const[0], warm0, free0)]
    L.rh_array_statics_solve_host(P(ri), P(rd), P(rec.point), P(rec.line), *[P(a) for a in args], P(X), P(warm), P(free),
                                  P(it), P(st))
    return X, free[:rec.nfree], int(it[0]), int(st[0])


@pytest.mark.parametrize("own", [False, True], ids=["array_only", "own_and_array"])
@pytest.mark.parametrize("key", C.KEYS)
def test_farm_statics_match_solve_statics(lib, key, own):
    """The host-compiled Newton against Model.solveStatics on a fresh model: X at 1e-9, equal
    evaluation counts, final free points; own=True gives FOWT 0 its own system beside the array's."""
    from raft.mooring import Point
    X, free, it, st = statics_host(lib, C.farm_model(key, own), C.CASES[key])
    m = C.farm_model(key, own)
    Xh = m.solveStatics(dict(C.CASES[key]))
    fh = np.array([p.r for p in m.ms.points if p.type == Point.FREE])
    print(f"farm {key} own={own}: max |dX| {np.abs(X - Xh).max():.3e}, evaluations {it} / {len(m.Xs2)}, "
          f"free points {np.abs(free - fh).max():.3e}")
    assert st == 0 and it == len(m.Xs2)
    np.testing.assert_allclose(X, Xh, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(free, fh, rtol=1e-9, atol=1e-9)
    if not own:
        from test_mooring import DESIRED_X0, FARM_MEASURED
        np.testing.assert_allclose(X, DESIRED_X0[key][2], rtol=FARM_MEASURED[key], atol=1e-10)


# ------------------------------------------------------------------------------ flattener
def test_flattener_tables_of_the_farm():
    from raft import _native as N
    from raft.mooring_array_device import FIXED, FREE, ON_BODY, array_state, flatten_array
    m = C.farm_model("wave", own=True)
    rec = flatten_array(m)
    own, arr = m.fowtList[0].ms, m.ms
    assert [ms for ms, _ in rec.systems] == [own, arr] and [list(b) for _, b in rec.systems] == [[0], [0, 1]]
    assert rec.nbody == 2 and rec.nfree == 2 and rec.free_sys == 1
    assert rec.nline == len(own.lines) + 7 and rec.npoint == len(own.points) + 12
    no = len(own.points)
    kinds = rec.point[N.MP["KIND"], no:].astype(int).tolist()
    assert kinds == [ON_BODY, FREE, FREE, ON_BODY, FIXED, ON_BODY, FIXED, ON_BODY, FIXED, ON_BODY, FIXED, ON_BODY]
    assert rec.point[N.MP["INDEX"], no:].astype(int).tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1]
    np.testing.assert_array_equal(rec.point[N.MP["X"]:N.MP["Z"] + 1, no], [58.0, 0.0, -14.0])        # body frame
    np.testing.assert_array_equal(rec.point[N.MP["X"]:N.MP["Z"] + 1, no + 3], [-58.0, 0.0, -14.0])
    np.testing.assert_array_equal(rec.point[N.MP["M"], no + 1:no + 3], [1e5, 1e5])
    assert set(rec.point[N.MP["KIND"], :no].astype(int)) == {FIXED, ON_BODY} and not rec.point[N.MP["INDEX"], :no].any()
    nl = len(own.lines)
    np.testing.assert_array_equal(rec.membership, [0] * nl + [1] * 7)
    np.testing.assert_array_equal(rec.line[N.MAL["DEPTH"]], [own.depth] * nl + [600.0] * 7)
    np.testing.assert_array_equal(rec.line[N.MAL["TOL"]], [own.cat_tol] * nl + [arr.cat_tol] * 7)
    np.testing.assert_array_equal(rec.line[N.MAL["A"], nl:] - no, [0, 1, 2, 4, 6, 8, 10])
    np.testing.assert_array_equal(rec.line[N.MAL["B"], nl:] - no, [1, 2, 3, 5, 7, 9, 11])
    np.testing.assert_array_equal(rec.line[N.MAL["L"], nl:], [150.0, 1168.0, 150.0, 1200.0, 1200.0, 1200.0, 1200.0])
    warm, free = array_state(rec)
    assert warm.shape == (rec.nline, 2) and free.shape == (2, 3) and (warm > 0).all()


# ------------------------------------------------------------------------------ refusals and limits
def no_device(monkeypatch):
    from raft import _native as N

    def touched(*a, **k):
        raise AssertionError("device touched before the refusal")
    monkeypatch.setattr(N, "lib", touched)
    monkeypatch.setattr(N, "context", touched)


def test_new_refusals(monkeypatch):
    """Each unsupported kind raises NotImplementedError by name before any device call."""
    from raft.mooring import Point
    from raft.mooring_array_device import DeviceArrayMooring
    no_device(monkeypatch)
    sysm = C.synthetic_systems()
    ms = sysm["clump"][0]
    ms.current = np.array([0.5, 0.0, 0.0])
    with pytest.raises(NotImplementedError, match="current"):
        DeviceArrayMooring([ms])
    ms = sysm["two_bodies"][0]
    ms.add_line_type("float", 0.2, 5.0, 1.0e8)
    assert ms.line_types["float"]["w"] < 0
    ms.add_line(900.0, "float", ms.points[0], ms.points[2])           # anchor to a fairlead
    with pytest.raises(NotImplementedError, match="buoyant"):
        DeviceArrayMooring([ms])
    ms = sysm["same_body"][0]
    ms.add_line(1700.0, "chain", ms.points[0], ms.points[1])           # anchor to anchor
    with pytest.raises(NotImplementedError, match="two fixed points"):
        DeviceArrayMooring([ms])
    a, b = C.synthetic_systems()["clump"][0], C.synthetic_systems()["chain8"][0]
    with pytest.raises(NotImplementedError, match="free points in more than one system"):
        DeviceArrayMooring([[(a, [0]), (b, [1])]])
    m = C.farm_model()                                                  # through the model, device untouched
    m.mooring_currentMod = 1
    with pytest.raises(NotImplementedError, match="current on the mooring lines"):
        m.solveStaticsArrayBatch([dict(C.CASES["current"])])
    m.mooring_currentMod = 0
    m.ms.points[1].type = Point.FIXED                                   # line 1-2 of the file now joins ...
    m.ms.points[2].type = Point.FIXED                                   # ... two fixed points
    with pytest.raises(NotImplementedError, match="two fixed points"):
        m.solveStaticsArrayBatch([dict(C.CASES["wave"])])


def test_limits(monkeypatch):
    """5 bodies, 9 free points and 65 lines are refused by name; 4, 8 and 64 flatten."""
    from raft.mooring import Point
    from raft.mooring_array_device import DeviceArrayMooring, flatten_array
    no_device(monkeypatch)

    def star(nbody, nline_per_body, nfree=0):
        ms = C._base()
        for ib in range(nbody):
            b = ms.add_body([1000.0 * ib, 0, 0, 0, 0, 0])
            for k in range(nline_per_body):
                th = 2 * np.pi * k / nline_per_body
                anchor = ms.add_point(Point.FIXED, [1000.0 * ib + 800 * np.cos(th), 800 * np.sin(th), -200.0])
                ms.add_line(850.0, "chain", anchor, C._fair(ms, b, [50 * np.cos(th), 50 * np.sin(th), -15.0]))
        prev = ms.points[0]
        for k in range(nfree):
            p = ms.add_point(Point.FREE, [700.0 - 10 * k, 5.0, -180.0], m=100.0)
            ms.add_line(20.0, "chain", prev, p)
            prev = p
        return ms
    assert flatten_array(star(4, 3)).nbody == 4
    with pytest.raises(NotImplementedError, match="5 bodies"):
        DeviceArrayMooring([star(5, 3)])
    assert flatten_array(star(1, 3, nfree=8)).nfree == 8
    with pytest.raises(NotImplementedError, match="9 free points"):
        DeviceArrayMooring([star(1, 3, nfree=9)])
    assert flatten_array(star(4, 16)).nline == 64
    with pytest.raises(NotImplementedError, match="65 lines"):
        DeviceArrayMooring([star(1, 65)])


def test_old_refusals_stand():
    """The single-body flattener and entry points still refuse a farm (tests/test_moor_host.py pins them)."""
    from raft.mooring_device import DeviceMooring, flatten
    m = C.farm_model()
    with pytest.raises(NotImplementedError):
        flatten(m.ms)
    with pytest.raises(NotImplementedError):
        DeviceMooring([m.ms])
    with pytest.raises(NotImplementedError):
        m.solveStaticsBatch([dict(C.CASES["wave"])])
    with pytest.raises(NotImplementedError):
        m.analyzeCasesBatch([dict(C.CASES["wave"])], statics=True)


# ------------------------------------------------------------------------------ dense solve
@pytest.mark.parametrize("n", [3, 6, 12, 24])
@pytest.mark.parametrize("nrhs", [1, 6])
def test_arr_lu_solve_matches_lapack(lib, n, nrhs):
    """arr_lu_solve (the n x n solve with several right-hand sides behind the free-point and
    condensation steps) against numpy.linalg.solve, as test_moor_host.test_solve6_matches_lapack does
    for solve6: rows scaled over nine decades and permuted from a row-dominant order (so the pivot
    search exchanges rows at most steps), a zero entry, a row stride ld > n + nrhs whose padding must
    come back untouched, and a singular matrix that returns false."""
    rng = np.random.default_rng(100 * n + nrhs)
    ld = n + nrhs + 3
    for _ in range(20):
        A = rng.normal(size=[n, n]) + 4.0 * np.sqrt(n) * np.eye(n)
        A = A[rng.permutation(n)] * 10 ** rng.uniform(-3, 6, size=[n, 1])
        A[rng.integers(n), rng.integers(n)] = 0.0
        B = rng.normal(size=[n, nrhs])
        M = np.full([n, ld], 7.25)
        M[:, :n], M[:, n:n + nrhs] = A, B
        assert lib.rh_moor_array_lu_host(M.ctypes.data, n, nrhs, ld) == 1
        ref = np.linalg.solve(A, B)
        assert np.all(M[:, n + nrhs:] == 7.25)
        assert np.abs(M[:, n:n + nrhs] - ref).max() <= 1e-12 * np.linalg.cond(A) * np.abs(ref).max()
    M = np.full([n, ld], 7.25)
    M[:, :n] = rng.normal(size=[n, n])
    M[:, n // 2] = 0.0                      # a zero column: an exactly zero pivot at step n // 2
    M[:, n:n + nrhs] = rng.normal(size=[n, nrhs])
    assert lib.rh_moor_array_lu_host(M.ctypes.data, n, nrhs, ld) == 0
    M[:, :n] = 0.0
    assert lib.rh_moor_array_lu_host(M.ctypes.data, n, nrhs, ld) == 0


# ------------------------------------------------------------------------------ ABI
def test_abi_exports_the_new_calls():
    import __graft_entry__ as g
    g.build()
    from raft import _native as N
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB], capture_output=True, text=True, check=True).stdout
    for sym in ["rh_moor_array_eval", "rh_array_statics_solve", "rh_array_solve_stats_ext"]:
        assert f" T {sym}\n" in out, sym
    L = N.lib()
    assert L.rh_version() == 8
    null = [None] * 12
    assert L.rh_moor_array_eval(None, None, None, 1, 1, *null[:11]) == N.RH_EINVAL
    assert b"null context" in L.rh_last_error()
    assert L.rh_array_statics_solve(None, None, None, 1, 1, *null[:12]) == N.RH_EINVAL
    assert b"null context" in L.rh_last_error()
    assert L.rh_array_solve_stats_ext(None, None, 1, 2, 1, None, None, None, 0, None, 1.0, None, None, None) == N.RH_EINVAL
    assert N.MOOR_STATUS[8].startswith("free-point equilibrium") and N.MOOR_STATUS[9].startswith("singular free-point")

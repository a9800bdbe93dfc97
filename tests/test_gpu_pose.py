"""GPU: per-case offset-pose designs and current loads on the device (csrc/rh_pose.hip through
raft/pose_device.py, Model.solveStaticsBatch(current_device=True) and analyzeCasesBatch(statics=True,
pose_device=True)).  The two kernels against the host build of the same header at the bounds of
tests/helpers/pose_cases.py (143, 51 and 149 nodes: partial passes of the 256-wide node sweep, one to three
64-node chunks, 68 poses with 5 to 13 distinct node counts each); the keywords against the per-case host
path at the project's device parity convention (1e-9 of each array's largest entry).  References are
computed once per module and shared."""
import os
import sys

import numpy as np
import pytest

from conftest import load_design
from test_gpu_moor import DYN_CASES, SEA, model40
from test_moor_host import CASES

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pose_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9                       # device parity convention: of each array's largest entry


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def lib():
    return PC.host_lib()


def device_designs(rec, X):
    T = rec.pose_tables(X)
    return PC.split_slabs(T["node"].cpu().numpy(), T["memb"].cpu().numpy(), T["mstart"].cpu().numpy(), T["nn"], T["nm"],
                          rec.nnode, rec.nmemb)


# ------------------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("name", PC.DESIGNS)
def test_pose_designs_match_host_build(lib, name):
    from raft.pose_device import PoseRecord, host_record
    f = PC.fowt_at_reference(name)
    X = PC.poses()
    host = host_record(f)
    rec = PoseRecord(f, 0, host=host)
    got = device_designs(rec, X)
    ref = PC.host_designs(lib, host, X)
    assert [t.shape[1] for t, _, _ in got] == [t.shape[1] for t, _, _ in ref]
    worst = PC.compare_designs(got, ref, name)
    print(f"{name}: rh_pose_designs vs the host build, in units of the bounds: {worst}; nn "
          f"{sorted({t.shape[1] for t, _, _ in got})}")
    one = device_designs(rec, X[:1])[0]
    for a, b in zip(one, got[0]):        # a pose's bits do not depend on the launch it is in
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", PC.DESIGNS)
def test_current_loads_match_long_double(name):
    from raft.pose_device import PoseRecord
    f = PC.fowt_at_reference(name)
    cases = PC.current_cases()
    ref = [PC.current_longdouble(f, c) for c in cases]
    rec = PoseRecord(f, 0)

    def run(cs):
        return rec.current_loads(f.r6, [c["current_speed"] for c in cs], [c["current_heading"] for c in cs], f.depth,
                                 f._current_zref(), f.shearExp_water, f.rho_water).cpu().numpy()
    D = run(cases)
    print(f"{name}: rh_current_loads residual / bound {PC.check_current(D, ref, name):.3f}")
    assert not D[-1].any()                                        # the zero-speed case
    np.testing.assert_array_equal(run(cases[:1])[0], D[0])        # a case's bits do not depend on its neighbours
    np.testing.assert_array_equal(f.currentLoadsBatch(cases, 0), D)


def test_argument_checks():
    import ctypes
    from raft import _native as N
    from raft.pose_device import PoseRecord
    f = PC.fowt_at_reference("OC3spar_test")
    rec = PoseRecord(f, 0)
    with pytest.raises(ValueError, match="pure translation"):
        rec.current_loads([0, 0, 0, 0.01, 0, 0], [1.0], [0.0], f.depth, 0.0, f.shearExp_water, f.rho_water)
    bad = N.RhPoseRecord.from_buffer_copy(rec.rec)
    bad.nnode = N.POSE_MAX_NODES + 1
    rc = N.lib().rh_pose_designs(N.context(0), ctypes.byref(bad), 1, *([None] * 7))
    assert rc == N.RH_EINVAL and b"nnode=1025" in N.lib().rh_last_error()
    bad = N.RhPoseRecord.from_buffer_copy(rec.rec)
    bad.nnode = rec.nnode - 1                                    # mstart no longer ends at nnode
    rc = N.lib().rh_pose_designs(N.context(0), ctypes.byref(bad), 1, *([None] * 7))
    assert rc == N.RH_EINVAL and b"mstart" in N.lib().rh_last_error()
    assert N.lib().rh_version() == 8


# ------------------------------------------------------------------------------ the keywords
MORE = [dict(CASES["current"], current_speed=1.1, current_heading=70, **SEA),
        dict(CASES["current"], current_speed=0.3, current_heading=-120, wave_period=12, wave_height=6, wave_heading=45)]
KEYS = ("mean_offsets", "Tmoor_avg", "Tmoor_std", "Tmoor_PSD", "psd", "std")


def test_statics_batch_current_device():
    cases = [dict(c) for c in DYN_CASES + MORE]
    a = model40().solveStaticsBatch([dict(c) for c in cases], current_device=True)
    m = model40()
    b = m.solveStaticsBatch([dict(c) for c in cases])
    assert not a["status"].any() and set(a) == set(b)
    print(f"solveStaticsBatch current_device: |X - X_host path| / max {rel(a['X'], b['X']):.2e}, evaluations {a['iters']}")
    np.testing.assert_array_equal(a["iters"], b["iters"])
    assert rel(a["X"], b["X"]) < TOL
    # the defaults run the code they ran
    c = m.solveStaticsBatch([dict(c) for c in cases], current_device=False, rotor_device=False)
    for k in b:
        np.testing.assert_array_equal(b[k], c[k], err_msg=k)


def compare_analyses(a, b, m):
    assert set(a) == set(b), set(a) ^ set(b)
    err = np.linalg.norm(a["Xi"] - b["Xi"], axis=(1, 2)) / np.linalg.norm(b["Xi"], axis=(1, 2))
    print(f"pose_device vs per-case designs: Xi residuals {err}, drag iterations {a['iters']} / {b['iters']}, closest "
          f"calls of the convergence test {a['margin']} / {b['margin']}")
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["statics_iters"], b["statics_iters"])
    assert not a["statics_status"].any() and np.all(a["status"] >= 0)
    assert err.max() < TOL
    for k in KEYS:
        assert rel(a[k], b[k]) < TOL, (k, rel(a[k], b[k]))
    f = m.fowtList[0]
    np.testing.assert_array_equal(f.r6, [f.x_ref, f.y_ref, 0, 0, 0, 0])      # left at the reference pose
    for mem in f.memberList:
        np.testing.assert_array_equal(mem.rA, f.r6[:3] + mem.rA0)


WANT = ("psd", "std", "zeta", "B_drag", "margin")


def test_analyze_cases_batch_pose_device():
    cases = DYN_CASES + MORE
    m = model40()
    a = m.analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=2, pose_device=True, want=WANT)
    b = model40().analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=2, want=WANT)
    assert len(set(a["iters"])) > 1 or a["iters"][0] > 1
    compare_analyses(a, b, m)
    # a second call on the same model (the cached record) gives the same bits
    a2 = m.analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=3, pose_device=True, want=WANT)
    for k in a:
        np.testing.assert_array_equal(a[k], a2[k], err_msg=k)


def aero40():
    import raft
    d = load_design("VolturnUS-S_aero")
    d["settings"].update(min_freq=0.01, max_freq=0.4)
    return raft.Model(d)


def test_analyze_cases_batch_pose_device_with_rotor():
    cases = [dict(CASES["wind_wave_current"]), dict(CASES["wave"])]      # an operating rotor, and the shared M / B
    m = aero40()
    a = m.analyzeCasesBatch([dict(c) for c in cases], statics=True, rotor_device=True, pose_device=True, want=WANT)
    b = aero40().analyzeCasesBatch([dict(c) for c in cases], statics=True, rotor_device=True, want=WANT)
    compare_analyses(a, b, m)


def test_defaults_are_unchanged():
    cases = [dict(c) for c in DYN_CASES]
    a = model40().analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=2)
    b = model40().analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=2, pose_device=False)
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_refusals_by_message():
    from test_pose_host import test_pose_device_refusals
    test_pose_device_refusals()

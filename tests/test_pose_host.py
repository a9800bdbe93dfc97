"""CPU check of the device pose-design and current-load restatement (raft-teststuff_amd/csrc/rh_pose.h)
against the Python it restates (Member.setPosition, prep.node_table, FOWT.calcCurrentLoads): the header
is compiled for the host with g++ (tools/pose_host.cpp), so the frame, node and current-load code the
GPU runs is compared here without a GPU.  Designs, poses, references and bounds: tests/helpers/pose_cases.py.
Also the host-side refusals of the pose_device / current_device keywords and the two new ABI symbols."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_design

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pose_cases as PC  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return PC.host_lib()


_PY = {}


def python_reference(name):
    if name not in _PY:
        _PY[name] = PC.python_designs(PC.fowt_at_reference(name), PC.poses())
    return _PY[name]


def test_pose_set_exercises_the_compaction():
    """The properties the pose set was chosen for, on the Python tables: many distinct node counts, both
    member counts on the spar, and no node near enough to the waterline for rounding to flip it."""
    want = {"VolturnUS-S_test": (11, 48, 61), "OC3spar_test": (5, 24, 31), "VolturnUS-S_rectcols": (13, 49, 67)}
    for name in PC.DESIGNS:
        f = PC.fowt_at_reference(name)
        assert sum(m.ns for m in f.memberList) == PC.NNODE[name]
        ref = python_reference(name)
        nn = [t.shape[1] for t, _, _ in ref]
        assert (len(set(nn)), min(nn), max(nn)) == want[name], (name, sorted(set(nn)))
        if name == "OC3spar_test":
            assert {m.shape[1] for _, m, _ in ref} == {1, 2}
    f = PC.fowt_at_reference("VolturnUS-S_rectcols")
    assert any(m.gamma == 25 for m in f.memberList) and {m.shape for m in f.memberList} == {"circular", "rectangular"}


@pytest.mark.parametrize("name", PC.DESIGNS)
def test_pose_designs_match_node_table(lib, name):
    from raft.pose_device import host_record
    f = PC.fowt_at_reference(name)
    X = PC.poses()
    # the guard first: no node of any pose sits within rounding of the waterline
    zmin = min(np.abs(np.array([m.rA0, m.rB0])).min() for m in f.memberList)
    r0 = f.r6.copy()
    near = np.inf
    for x in X:
        f.setPosition(x)
        near = min(near, min(np.abs(m.r[:, 2]).min() for m in f.memberList))
    f.setPosition(r0)
    assert near > 1e-6, (near, zmin)
    got = PC.host_designs(lib, host_record(f), X)
    worst = PC.compare_designs(got, python_reference(name), name)
    print(f"{name}: closest node to z = 0 {near:.2e} m; host build vs node_table, in units of the bounds: {worst}")


@pytest.mark.parametrize("name", PC.DESIGNS)
def test_current_loads_match_long_double(lib, name):
    from raft.pose_device import host_record
    f = PC.fowt_at_reference(name)
    cases = PC.current_cases()
    ref = [PC.current_longdouble(f, c) for c in cases]
    D_host = PC.host_current_loads(lib, host_record(f), f, cases)
    D_py = np.array([f.calcCurrentLoads(dict(c)) for c in cases])
    w_host, w_py = PC.check_current(D_host, ref, f"{name} host build"), PC.check_current(D_py, ref, f"{name} calcCurrentLoads")
    print(f"{name}: residual / bound, host build {w_host:.3f}, calcCurrentLoads {w_py:.3f}")
    assert np.abs(D_py[:-1]).max() > 1e3 and not D_host[-1].any() and not D_py[-1].any()      # (a load; the zero-speed case)


def test_zero_pose_frame_is_what_set_position_rotates():
    from raft.hydro_math import rotation_matrix
    f = PC.fowt_at_reference("VolturnUS-S_rectcols")
    x = PC.poses()[66]
    r0 = f.r6.copy()
    f.setPosition(x)
    Rp = rotation_matrix(*x[3:])
    for m in f.memberList:
        _, q, p1, p2 = m.zero_pose_frame()
        np.testing.assert_array_equal(m.q, Rp @ q)
        np.testing.assert_array_equal(m.p1, Rp @ p1)
        np.testing.assert_array_equal(m.p2, Rp @ p2)
    f.setPosition(r0)


def test_abi_symbols_and_version():
    hdr = open(os.path.join(ROOT, "include", "rafthip.h")).read()
    src = open(os.path.join(ROOT, "raft-teststuff_amd", "csrc", "rh_pose.hip")).read()
    for sym in ("rh_pose_designs", "rh_current_loads"):
        assert f"int {sym}(" in hdr and f"int {sym}(" in src
    from raft import _native as N
    assert N.PM_COUNT == 16 and "RH_PM_COUNT" in hdr
    assert "int rh_version(void) { return 8; }" in open(os.path.join(ROOT, "raft-teststuff_amd", "csrc", "rh_abi.hip")).read()


# ------------------------------------------------------------------------------ refusals (host side: no device call)
def model40(name="VolturnUS-S_test"):
    import raft
    d = load_design(name)
    d["settings"].update(min_freq=0.01, max_freq=0.4)
    return raft.Model(d)


WAVE = dict(wind_speed=0, wind_heading=0, turbulence=0, turbine_status="operating", yaw_misalign=0,
            wave_spectrum="JONSWAP", wave_period=10, wave_height=4, wave_heading=-30, current_speed=0, current_heading=0)


def test_pose_device_refusals():
    m = model40()
    with pytest.raises(ValueError, match="pose_device=True needs statics=True"):
        m.analyzeCasesBatch([dict(WAVE)], pose_device=True)
    m.fowtList[0].memberList[0].MCF = True
    with pytest.raises(NotImplementedError, match="MacCamy-Fuchs"):
        m.analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True)
    m = model40()
    m.fowtList[0].potModMaster = 2
    with pytest.raises(NotImplementedError, match="BEM excitation"):
        m.analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True)
    m = model40()
    m.fowtList[0].potSecOrder = 1
    with pytest.raises(NotImplementedError, match="potSecOrder"):
        m.analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True)
    with pytest.raises(ValueError, match="pose_chunk"):
        model40().analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True, pose_chunk=0)
    import raft
    farm = raft.Model(load_design("VolturnUS-S_farm"))
    with pytest.raises(NotImplementedError, match="arrays"):
        farm.analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True)
    # the refusals of the other device keywords with statics=True stand
    with pytest.raises(NotImplementedError, match="aero_device=True with statics=True"):
        model40().analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True, aero_device=True)
    with pytest.raises(NotImplementedError, match="channels=True with statics=True"):
        model40().analyzeCasesBatch([dict(WAVE)], statics=True, pose_device=True, channels=True)
